"""bench.py's input writers (not the product): the single-member gzip stream of `--e2e-gzip` and the BGZF container of
`--e2e-bgzf` must be valid files of their kind, or the end-to-end numbers measure an error path."""
import gzip
import os
import sys
import zlib

import numpy as np
import pytest

import helpers as H

sys.path.insert(0, H.ROOT)
import bench  # noqa: E402


def test_crc32_combine():
    rng = np.random.default_rng(1)
    for la, lb in ((0, 0), (1, 0), (0, 5), (7, 1), (1000, 33), (65536, 100001)):
        a = bytes(rng.integers(0, 256, la, dtype=np.uint8))
        b = bytes(rng.integers(0, 256, lb, dtype=np.uint8))
        assert bench._crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b)


def test_gzip_one_stream_is_one_valid_member(tmp_path):
    rng = np.random.default_rng(2)
    data = b">c\n" + bytes(rng.choice(np.frombuffer(b"ACGT\n", dtype=np.uint8), 3_000_000))
    src, dst = str(tmp_path / "d.fa"), str(tmp_path / "d.fa.gz")
    with open(src, "wb") as f:
        f.write(data)
    bench.gzip_one_stream(src, dst, 2)
    with gzip.open(dst, "rb") as f:
        assert f.read() == data
    with open(dst, "rb") as f:
        z = f.read()
    d = zlib.decompressobj(31)
    assert d.decompress(z) == data and d.eof and d.unused_data == b""  # ONE member, nothing behind it


def test_bgzf_writer(tmp_path):
    rng = np.random.default_rng(3)
    data = b">c\n" + bytes(rng.choice(np.frombuffer(b"ACGT\n", dtype=np.uint8), 500_000))
    src, dst = str(tmp_path / "d.fa"), str(tmp_path / "d.fa.gz")
    with open(src, "wb") as f:
        f.write(data)
    bench.bgzf_compress(src, dst, 2)
    with gzip.open(dst, "rb") as f:
        assert f.read() == data
    with open(dst, "rb") as f:
        head = f.read(18)
    assert head[:4] == b"\x1f\x8b\x08\x04" and head[12:14] == b"BC"  # a BGZF member: FEXTRA with the BC subfield
    assert os.path.getsize(dst) > 0


def _records(n, n_contigs, seed):
    from ntedit_amd import _lib
    rng = np.random.default_rng(seed)
    recs = np.zeros(n, dtype=np.dtype(_lib.EDIT_DTYPE))
    recs["contig"] = np.sort(rng.integers(0, n_contigs, n))
    recs["draft_pos"] = rng.integers(0, 50_000_000, n)
    recs["kind"] = rng.integers(1, 5, n)
    indel = (recs["kind"] == _lib.EDIT_INS) | (recs["kind"] == _lib.EDIT_DEL)
    recs["len"] = np.where(indel, rng.integers(1, 6, n), 1)
    recs["support"] = rng.integers(0, 300, n)
    recs["draft_base"] = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), n)
    recs["new_base"] = np.where(indel, 0, rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))
    recs["n_alt"] = rng.integers(0, 4, n)
    recs["alt_base"] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (n, 3))
    recs["alt_support"] = rng.integers(0, 256, (n, 3))
    pool = bytearray()
    for i in range(n):  # (the renderer's layout: an indel's bases appended in record order, bases_off = pool size)
        recs["bases_off"][i] = len(pool)
        if indel[i]:
            pool += bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), recs["len"][i]))
    return recs, bytes(pool)


def _stats():
    import types
    return types.SimpleNamespace(**{f: 10 * i + 3 for i, f in enumerate(bench.STATS_FIELDS)})


def _npy_sizes(d):
    return {p.name: p.stat().st_size for p in d.iterdir()}


def test_dump_edits_writes_every_record_when_they_fit(tmp_path):
    from ntedit_amd import _lib
    recs, pool = _records(5000, 7, 4)
    bench.dump_edits(str(tmp_path), recs, pool, _stats(), 9)
    got = {p.stem: np.load(p) for p in tmp_path.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["stats"].tolist() == [10.0 * i + 3 for i in range(len(bench.STATS_FIELDS))]
    assert got["edits_per_contig"].tolist() == np.bincount(recs["contig"], minlength=9).tolist()
    assert got["edits_per_kind"].tolist() == np.bincount(recs["kind"], minlength=5).tolist()
    assert got["edit_index"].tolist() == list(range(len(recs)))
    for f in ("contig", "draft_pos", "len", "support", "kind", "draft_base", "new_base", "n_alt", "alt_base", "alt_support"):
        assert np.array_equal(got["edit_" + f], recs[f]), f
    want = b"".join(pool[r["bases_off"]:r["bases_off"] + r["len"]] for r in recs
                    if r["kind"] in (_lib.EDIT_INS, _lib.EDIT_DEL))
    assert len(want) > 1000 and bytes(got["edit_bases"].astype(np.uint8)) == want


def test_dump_edits_samples_within_the_limit_the_same_way_every_time(tmp_path):
    recs, pool = _records(20000, 3, 5)
    limit = 256 << 10
    for d in ("a", "b"):
        bench.dump_edits(str(tmp_path / d), recs, pool, _stats(), 3, prefix="rank1_", limit=limit)
        assert sum(_npy_sizes(tmp_path / d).values()) <= limit
    a = {p.name: np.load(p) for p in (tmp_path / "a").iterdir()}
    b = {p.name: np.load(p) for p in (tmp_path / "b").iterdir()}
    assert sorted(a) == sorted(b) and all(n.startswith("rank1_") for n in a)
    assert all(np.array_equal(a[n], b[n]) for n in a)
    idx = a["rank1_edit_index.npy"].astype(np.int64)
    assert 1000 < len(idx) < len(recs) and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["rank1_edit_draft_pos.npy"], recs["draft_pos"][idx])
    assert a["rank1_edits_per_contig.npy"].sum() == len(recs)  # (the per-contig counts cover every record)
    from ntedit_amd import _lib
    want = b"".join(pool[r["bases_off"]:r["bases_off"] + r["len"]] for r in recs[idx]
                    if r["kind"] in (_lib.EDIT_INS, _lib.EDIT_DEL))
    assert bytes(a["rank1_edit_bases.npy"].astype(np.uint8)) == want


def test_dump_edits_of_an_empty_result(tmp_path):
    recs, pool = _records(0, 1, 6)
    bench.dump_edits(str(tmp_path), recs, pool, _stats(), 4)
    assert np.load(tmp_path / "edit_index.npy").shape == (0,)
    assert np.load(tmp_path / "edits_per_contig.npy").tolist() == [0.0] * 4


def test_dump_screen(tmp_path):
    rng = np.random.default_rng(7)
    n = 300_000 + 13
    words = rng.integers(0, 2 ** 63, (n + 63) // 64 + 1, dtype=np.int64)  # (one spare word, as bench.py allocates it)
    bench.dump_screen(str(tmp_path), words, n)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
    per_block = np.load(tmp_path / "screen_absent_per_block.npy")
    assert per_block.dtype == np.float64 and per_block.tolist() == [float(bits[i:i + 65536].sum()) for i in range(0, n, 65536)]
    idx = np.load(tmp_path / "screen_word_index.npy").astype(np.int64)
    assert idx.tolist() == list(range((n + 63) // 64))
    lo, hi = np.load(tmp_path / "screen_word_lo.npy"), np.load(tmp_path / "screen_word_hi.npy")
    full = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    assert np.array_equal(full[:-1], words[:len(idx) - 1].view(np.uint64))
    assert np.unpackbits(full[-1:].view(np.uint8), bitorder="little").sum() == bits[(len(idx) - 1) * 64:].sum()
    bench.dump_screen(str(tmp_path / "s"), words, n, limit=64 << 10)
    assert sum(_npy_sizes(tmp_path / "s").values()) <= 64 << 10


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_a_plain_run_leaves_the_extra_measurements_to_full(monkeypatch):
    assert not _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5").full
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--e2e-bgzf")
    assert a.full and a.no_cpu_baseline and a.e2e_bgzf


def test_compressed_end_to_end_options_need_full(monkeypatch, capsys):
    for opt in ("--e2e-gzip", "--e2e-bgzf"):
        with pytest.raises(SystemExit) as e:
            _parse(monkeypatch, opt)
        assert e.value.code == 2 and "--full" in capsys.readouterr().err
