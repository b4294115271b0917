"""ntedit_amd/host/chunk_feed.h on the CPU: tests/feed/feed_host.cpp runs the queue, the three producers and the overlap
loop with malloc behind the page-locked allocator, built plain, with -fsanitize=address,undefined and with
-fsanitize=thread.  The inputs are written here (files of a few KB, batches of 64 to 1,000 bytes: the feeders have no
4,096 floor), and every chunk list the program prints is compared with a restatement of its cut rule written here.
No GPU, nothing of the library linked; the exported ntedit_hip_reads_last_record_start must agree with the moved rule."""
import os
import random
import re
import struct
import subprocess

import pytest

import bgzf_corpus as BC
import helpers as H

_SRC = os.path.join(H.ROOT, "tests", "feed", "feed_host.cpp")
_FLAGS = {"plain": ["-O2"],
          "asan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
          "tsan": ["-O1", "-g", "-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(_FLAGS))
def exe(request, tmp_path_factory):
    """g++ build of the host program (as test_draw_cpu.build_draw_host), once per flavour"""
    out = str(tmp_path_factory.mktemp("feed") / ("feed_host_" + request.param))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-pthread"] + _FLAGS[request.param] + ["-o", out, _SRC], check=True)
    return out


def run(exe, *args):
    """stdout of one run; any sanitizer report fails it (a report ends the program with a non-zero status)"""
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=120)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (args, r.returncode, err[-4000:])
    return r.stdout


# ------------------------------------------------------------------ the queue and the overlap loop
@pytest.mark.parametrize("n", [0, 1, 2, 3, 1000])
def test_every_chunk_arrives_once_in_order(exe, n):
    lines = run(exe, "queue", n).decode().splitlines()
    want = ["chunk %d last %d byte %d" % (i, i == n - 1, i & 255) for i in range(n)]
    assert lines == want + (["end at last"] if n else ["end error ''"])


def test_the_consumer_leaves_while_the_producer_waits_for_a_buffer(exe):
    assert run(exe, "abandon").decode().splitlines() == ["chunk 0", "chunk 1", "abandoned"]


def test_queued_chunks_are_handed_out_before_a_failure(exe):
    assert run(exe, "queue", 2, "fail").decode().splitlines() == ["chunk 0 last 0 byte 0", "chunk 1 last 0 byte 1", "end error 'boom'"]
    assert run(exe, "queue", 0, "fail").decode().splitlines() == ["end error 'boom'"]


@pytest.mark.parametrize("n, stop_at, fail_at, begin_fail_at, rc, begun, worked", [
    (0, -1, -1, -1, 0, 0, 0), (1, -1, -1, -1, 0, 1, 1), (5, -1, -1, -1, 0, 5, 5), (200, -1, -1, -1, 0, 200, 200),
    (5, 1, -1, -1, 1, 3, 2),    # the work hands back at chunk 1: the copy of chunk 2 is in flight
    (5, 4, -1, -1, 1, 5, 5),    # ... at the last chunk
    (5, -1, 1, -1, -5, 3, 1),   # the work fails at chunk 1 before it waited for its own copy: two in flight
    (5, -1, 0, -1, -5, 2, 0),
    (5, -1, -1, 0, -2, 0, 0),   # the first copy cannot begin
    (5, -1, -1, 2, -2, 2, 1),   # the copy of chunk 2 cannot begin while chunk 1's is in flight
])
def test_no_buffer_is_freed_or_refilled_while_a_copy_reads_it(exe, n, stop_at, fail_at, begin_fail_at, rc, begun, worked):
    """the overlap loop against a pretended copy engine; the program counts a buffer freed, or back with the producer,
    while its copy has not been waited for"""
    out = run(exe, "overlap", n, stop_at, fail_at, begin_fail_at).decode().strip()
    assert out == "overlap rc %d begun %d worked %d violations 0" % (rc, begun, worked)


# ------------------------------------------------------------------ parsed batches
def test_batches_and_their_growth_rule(exe, tmp_path):
    rng = random.Random(5)
    seqs = ["".join(rng.choice("ACGT") for _ in range(rng.choice((3, 20, 40, 90, 150)))) for _ in range(200)] + ["A" * 700, "C" * 30]
    (tmp_path / "seqs.txt").write_text("\n".join(seqs) + "\n")
    k, batch = 25, 256
    out = run(exe, "batch", tmp_path / "seqs.txt", k, batch)
    # the restatement: reads of k bases or more, each followed by '\n'; a read that would pass batch_bytes starts a new batch
    want, cur = [], b""
    for s in seqs:
        if len(s) < k:
            continue
        if cur and len(cur) + len(s) + 1 > batch:
            want.append(cur)
            cur = b""
        cur += s.encode() + b"\n"
    want.append(cur)
    at = 0
    for i, text in enumerate(want):
        head = b"batch len %d bases %d last %d\n" % (len(text), len(text) - text.count(b"\n"), i == len(want) - 1)
        assert out[at:at + len(head) + len(text)] == head + text, i
        at += len(head) + len(text)
    # a buffer is max(need, batch_bytes) bytes: two of 256, and one that grew for the read of 700
    assert out[at:].decode().split() == ["allocs", "256", "256", "701"]


# ------------------------------------------------------------------ raw chunks
def fasta(rng, n):
    return b"".join(b">r%d x\n%s\n" % (i, "".join(rng.choice("ACGT") for _ in range(rng.randrange(1, 60))).encode()) for i in range(n))


def fastq(rng, n, tricky=False):
    out = b""
    for i in range(n):
        s = "".join(rng.choice("ACGT") for _ in range(rng.randrange(1, 60)))
        q = ("@" if tricky else "I") + "".join(rng.choice("@+I5") for _ in range(len(s) - 1))
        out += b"@r%d\n%s\n+%s\n%s\n" % (i, s.encode(), b"" if tricky else b"r%d" % i, q.encode())
    return out


def records_rule(data, start, stop, batch):
    """[(off, len)]: about `batch` bytes are read behind the carried tail; the chunk ends at the last record start within
    them (another batch is read when there is none), the range's last chunk where the range does"""
    chunks, pos, tail = [], start, 0
    while pos < stop:
        want = batch if batch > tail else tail + batch
        while True:
            want = min(want, stop - pos)
            buf = data[pos:pos + want]
            if pos + want == stop:
                cut = want
            else:
                cut = BC.python_last_record_start(buf, buf[0]) if buf[:1] in (b">", b"@") else want
            if cut is not None:
                break
            want += batch
        chunks.append((pos, cut))
        tail = want - cut
        pos += cut
    return chunks


def raw_chunks(exe, tmp_path, data, start, stop, batch, rule):
    (tmp_path / "in").write_bytes(data)
    out = run(exe, "raw", tmp_path / "in", start, stop, batch, rule, tmp_path / "out").decode().splitlines()
    assert out[-2] == "end error ''"
    chunks = [tuple(int(x) for x in re.fullmatch(r"chunk off (\d+) len (\d+) last (\d)", l).groups()) for l in out[:-2]]
    assert (tmp_path / "out").read_bytes() == data[start:stop]  # the chunks concatenate to the range
    assert [c[2] for c in chunks] == [0] * (len(chunks) - 1) + [1] * bool(chunks)  # `last` on the last one only
    at = start
    for off, n, _ in chunks:  # `off` runs on
        assert off == at
        at += n
    return [(off, n) for off, n, _ in chunks], [int(x) for x in out[-1].split()[1:]]


def test_raw_chunks_are_cut_at_record_starts(exe, tmp_path):
    rng = random.Random(11)
    long_record = b">long\n" + b"ACGT" * 200 + b"\n"  # longer than three batches of 200: the chunk grows
    inputs = {"fasta": fasta(rng, 200), "fastq": fastq(rng, 200), "tricky fastq": fastq(rng, 200, tricky=True),
              "long record": fasta(rng, 10) + long_record + fasta(rng, 10)}
    for name, data in inputs.items():
        for batch in (64, 200, 1000):
            got, allocs = raw_chunks(exe, tmp_path, data, 0, len(data), batch, "records")
            assert got == records_rule(data, 0, len(data), batch), (name, batch)
            assert len(got) > 2 and allocs[0] == batch
    # every chunk but the first starts a record, and the FASTQ cut is never fooled by a quality line that starts with '@'
    data = inputs["tricky fastq"]
    starts = {m.start() for m in re.finditer(rb"(?m)^@r\d+\n", data)}
    assert {off for off, _ in raw_chunks(exe, tmp_path, data, 0, len(data), 64, "records")[0]} <= starts
    # a range inside the file, from a record start to a record start
    data = inputs["fasta"]
    recs = [m.start() for m in re.finditer(rb"(?m)^>", data)]
    for start, stop in ((recs[7], recs[150]), (recs[0], recs[1]), (recs[199], len(data))):
        assert raw_chunks(exe, tmp_path, data, start, stop, 100, "records")[0] == records_rule(data, start, stop, 100)
    # the grown chunk: one chunk holds the long record whole, in a buffer that grew by a batch at a time
    data = inputs["long record"]
    got, allocs = raw_chunks(exe, tmp_path, data, 0, len(data), 200, "records")
    assert any(n > 800 for _, n in got) and max(allocs) > 800 and all(a % 200 == 0 or a == max(allocs) for a in allocs)


def test_the_exported_cut_rule_agrees_with_the_moved_one(exe, tmp_path):
    from ntedit_amd import _lib
    lib = _lib.load()
    rng = random.Random(12)
    for kind, data in ((">", fasta(rng, 12)), ("@", fastq(rng, 8, tricky=True))):
        (tmp_path / "in").write_bytes(data)
        got = [int(x) for x in run(exe, "cut", tmp_path / "in", kind).split()]
        want = [lib.ntedit_hip_reads_last_record_start(data, n, ord(kind)) for n in range(1, len(data) + 1)]
        assert got == [-1 if w == _lib.READS_NO_START else w for w in want]
        assert len({g for g in got if g >= 0}) >= 6


def test_raw_chunks_cut_anywhere(exe, tmp_path):
    data = fasta(random.Random(13), 60)
    for size, batch in ((len(data), 100), (1000, 100), (100, 100), (99, 100), (101, 100), (1, 64), (0, 64)):
        got, allocs = raw_chunks(exe, tmp_path, data[:size], 0, size, batch, "anywhere")
        assert got == [(off, min(batch, size - off)) for off in range(0, size, batch)], (size, batch)
        assert allocs == [n for _, n in got[:2]]  # a chunk's exact size, once per buffer (no later chunk is longer)


# ------------------------------------------------------------------ BGZF chunks
def members_of(data):
    """the walk, restated: [(offset, size, ISIZE)] of the whole BGZF members from byte 0, and where they end"""
    out, o = [], 0
    while o + 18 <= len(data) and data[o:o + 4] == b"\x1f\x8b\x08\x04" and data[o + 10:o + 16] == b"\x06\0BC\x02\0":
        size = struct.unpack("<H", data[o + 16:o + 18])[0] + 1
        if size < 26 or o + size > len(data):
            break
        out.append((o, size, struct.unpack("<I", data[o + size - 4:o + size])[0]))
        o += size
    return out, o


def bgzf_rule(data, batch):
    """the chunks: whole members while their ISIZE sum stays within batch (at least one); the last chunk is the one behind
    which no whole member follows, and is not `whole` when the file does not end there"""
    members, end = members_of(data)
    chunks, i = [], 0
    while True:
        first, n_out = i, 0
        while i < len(members) and (i == first or n_out + members[i][2] <= batch):
            n_out += members[i][2]
            i += 1
        last = i == len(members)
        chunks.append((first, i - first, n_out, sum(m[1] for m in members[first:i]), int(last), int(not last or end == len(data))))
        if last:
            return chunks, members, end


def bgzf_chunks(exe, tmp_path, data, batch, how):
    (tmp_path / "in.gz").write_bytes(data)
    out = run(exe, "bgzf", tmp_path / "in.gz", batch, how, tmp_path / "out").decode().splitlines()
    assert out[-1] == "end error ''"
    chunks, table = [], []
    for l in out[:-1]:
        nums = tuple(int(x) for x in re.findall(r"\d+", l))
        if l.startswith("chunk"):
            chunks.append(nums)
            table.append([])
        else:
            table[-1].append(nums)
    return chunks, table, (tmp_path / "out").read_bytes()


def test_bgzf_chunks_are_whole_members_within_the_budget(exe, tmp_path):
    rng = random.Random(14)
    text = BC.fastq_text(rng, 40 * 500)
    files = {}
    for n in (1, 2, 40):
        for eof in (True, False):
            files["%d members eof %d" % (n, eof)] = BC.bgzf(text[:n * 500], block=500, eof=eof)
    forty = BC.bgzf(text, block=500, eof=True)
    files["trailing text"] = BC.bgzf(text, block=500, eof=False) + b"@r\nACGT\n+\nIIII\n"
    files["cut inside a member"] = forty[:len(forty) - 28 - 100]
    files["cut inside a header"] = forty[:len(forty) - 28 + 7]
    files["not BGZF"] = b"@r\nACGT\n+\nIIII\n" * 10
    files["many slabs"] = BC.bgzf(bytes(rng.getrandbits(8) for _ in range(40 * 8000)), block=8000, level=1)  # 320 KB, read in pieces
    for name, data in files.items():
        for batch in (64, 499, 500, 1000, 1500, 1 << 20) if name != "many slabs" else (8000, 20000):
            want, members, end = bgzf_rule(data, batch)
            chunks, table, comp = bgzf_chunks(exe, tmp_path, data, batch, "thread")
            assert chunks == want, (name, batch)
            assert comp == data[:end], (name, batch)  # the chunks' compressed bytes: the walked prefix of the file
            for (first, n, n_out, size, last, whole), ms in zip(chunks, table):
                assert n_out <= batch or n == 1
                in_off = out_off = 0
                for (off, msize, isize), m in zip(members[first:first + n], ms):  # offsets relative to the chunk
                    assert m[:4] == (in_off + 18, out_off, msize - 26, isize)
                    assert m[4] == struct.unpack("<I", data[off + msize - 8:off + msize - 4])[0]
                    in_off += msize
                    out_off += isize
            # ... and the same list without a thread
            assert bgzf_chunks(exe, tmp_path, data, batch, "serial") == (chunks, table, comp), (name, batch)
    last = lambda name, batch: bgzf_rule(files[name], batch)[0][-1]
    assert last("trailing text", 1000)[4:] == (1, 0) and last("cut inside a member", 1000)[4:] == (1, 0)
    assert last("40 members eof 1", 1000)[4:] == (1, 1) and bgzf_rule(files["not BGZF"], 64)[0] == [(0, 0, 0, 0, 1, 0)]
    assert [c[1] for c in bgzf_rule(files["40 members eof 0"], 499)[0]] == [1] * 40  # a batch below one member's ISIZE
    assert [c[1] for c in bgzf_rule(files["40 members eof 0"], 1500)[0]] == [3] * 13 + [1]  # a batch of exactly 3 members
