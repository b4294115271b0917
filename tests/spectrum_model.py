"""The numpy restatement of the k-mer multiplicity spectrum (include/ntedit_hip.h), on
reads_model.kmer_hashes: per sequence m = data[hv % counters].min(axis=1), the 256 bins and the three fields of the
entry's row.  The counting filters of the spectrum tests are made here as well, so that a test controls the multiplicities.
A plain module shared by the spectrum tests."""
import numpy as np

import reads_model as RM

ROW_DTYPE = np.dtype([("kmers", "<u8"), ("sum", "<u8"), ("saturated", "<u8")])


def multiplicities(seq, data, k, h):
    """m of every k-mer of ACGTacgt of one sequence, in order of position"""
    hv = RM.kmer_hashes(bytes(seq), k, h)
    if hv.shape[0] == 0:
        return np.zeros(0, dtype=np.uint8)
    return data[(hv % np.uint64(len(data))).astype(np.int64)].min(axis=1)


def spectrum(seqs, data, k, h):
    """(bins uint64[256], rows ROW_DTYPE[len(seqs)]) of a batch whose entries are `seqs`"""
    data = np.asarray(data, dtype=np.uint8)
    bins = np.zeros(256, dtype=np.uint64)
    rows = np.zeros(len(seqs), dtype=ROW_DTYPE)
    for i, s in enumerate(seqs):
        m = multiplicities(s, data, k, h)
        bins += np.bincount(m, minlength=256).astype(np.uint64)
        rows[i] = (m.size, int(m.astype(np.int64).sum()), int((m == 255).sum()))
    return bins, rows


def entries_of(blob, offs, lens):
    return [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(offs, lens)]


def brute_force(seq, data, k, h):
    """the definition, one k-mer at a time, in Python integers: (bins list, kmers, sum, saturated)"""
    M64 = RM.M64
    bins = [0] * 256
    code = {c: i for i, c in enumerate(b"ACGT")}
    code.update({c | 0x20: i for c, i in list(code.items())})
    total = sat = n = 0
    for p in range(len(seq) - k + 1):
        w = seq[p:p + k]
        if any(c not in code for c in w):
            continue
        fh = rh = 0
        for i, c in enumerate(w):
            fh ^= RM._sroln(RM.SEEDS[code[c]], k - 1 - i)
            rh ^= RM._sroln(RM.SEEDS[3 - code[c]], i)
        base = (fh + rh) & M64
        m = 255
        for i in range(h):
            hv = base
            if i:
                t = (base * (i ^ ((k * RM.MULTISEED) & M64))) & M64
                hv = t ^ (t >> RM.MULTISHIFT)
            m = min(m, int(data[hv % len(data)]))
        bins[m] += 1
        n += 1
        total += m
        sat += m == 255
    return bins, n, total, sat


def counting_filter(seqs, k, h, counters, est_of, cmin=1, pinned=()):
    """8-bit counters of a filter over the distinct k-mers of `seqs`: k-mer x is entered with the count est_of(i) of its
    index i in order of first appearance, a count below cmin not at all (reads_model.model_counts: every slot holds the
    largest count entered).  pinned: (sequence, count) pairs -- every k-mer of that sequence gets that count."""
    seqs = list(seqs) + [s for s, _ in pinned]
    hv = np.concatenate([RM.kmer_hashes(bytes(s), k, h) for s in seqs] + [np.zeros((0, h), dtype=np.uint64)])
    _, first = np.unique(hv[:, 0], return_index=True)
    hv = hv[np.sort(first)]
    est = np.asarray(est_of(np.arange(hv.shape[0])), dtype=np.int64).copy()
    for s, count in pinned:
        est[np.isin(hv[:, 0], RM.kmer_hashes(bytes(s), k, 1)[:, 0])] = count
    return RM.model_counts(hv, est, cmin, counters)


def check_not_degenerate(bins):
    """a filter that gave everything one multiplicity would let a test pass vacuously"""
    assert bins[0] > 0 and bins[255] > 0 and int((bins[1:255] > 0).sum()) >= 5, bins


def polish_case(tmp):
    """The small polish case of the spectrum, copy-number and apply tests, written under tmp (needs a GPU: the filter is saved
    through the library): H.make_case(.., 32001, "N lower") with a numpy counting filter over the truth's k-mers, every one
    entered with a count of 1 or more (1: absent at -p 2), one stretch at 255; the filter as a .bf file"""
    import os

    import helpers as H
    import ntedit_amd
    case = H.make_case(tmp, 32001, flavor="N lower")
    truth = [s for _, s in H.read_fasta(case["truth"])]
    k, h = 25, 3
    data = counting_filter(truth, k, h, 1 << 20, lambda i: 1 + (i * 7) % 60, pinned=[(truth[1][700:1400], 255)])
    hv = np.concatenate([RM.kmer_hashes(t, k, h) for t in truth])
    assert data[(hv % np.uint64(len(data))).astype(np.int64)].min() >= 1  # (all at least 1 on the truth's k-mers)
    recs = H.read_fasta(case["draft"])
    assert set(b"".join(s for _, s in recs)) <= set(b"ACGTNacgtn")
    pol = ntedit_amd.Polisher(0)
    try:
        pol.set_filter(data, h, k, counting=True)
        case["counts_bf"] = os.path.join(tmp, "counts.bf")
        pol.filter_save_file(case["counts_bf"])
    finally:
        pol.close()
    assert H.load_bf(case["counts_bf"])["counting"]
    case.update(tmp=tmp, recs=recs, k=k, h=h, data=data)
    return case
