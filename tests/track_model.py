"""The unsupported regions of a batch as intervals: a numpy model written from the definition alone (include/ntedit_hip.h,
DESIGN.md 9.12), not from the kernels.

A batch has n positions and entries e at [offs[e], offs[e] + lens[e]).  A position p is a marked start of entry e iff its
bit is set and offs[e] <= p < offs[e] + lens[e] - k + 1.  An interval of e is a maximal sequence of its marked starts
p1 < ... < pm in which consecutive starts are at most k apart; it never continues into another entry.  Its record is
(entry = e, begin = p1 - offs[e], end = pm - offs[e] + k, absent = m); records are ordered by entry, then by begin."""
import numpy as np

DTYPE = np.dtype([("entry", "<u4"), ("begin", "<u4"), ("end", "<u4"), ("absent", "<u4")])


def bits_of(words):
    """uint64 bitmap words -> one uint8 per position (position p = bit p % 64 of word p / 64)"""
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little")


def words_of(bits):
    """one value per position -> uint64 bitmap words, zero-padded to a whole word"""
    bits = np.asarray(bits, dtype=np.uint8)
    padded = np.zeros((len(bits) + 63) // 64 * 64, dtype=np.uint8)
    padded[:len(bits)] = bits != 0
    return np.packbits(padded, bitorder="little").view("<u8").copy()


def intervals(bits, offs, lens, k):
    """bits: one value per position (what lies behind the last entry is never looked at); returns records of DTYPE"""
    bits = np.asarray(bits)
    out = []
    for e, (o, l) in enumerate(zip(offs, lens)):
        o, l = int(o), int(l)
        if l < k:
            continue
        starts = o + np.flatnonzero(bits[o:o + l - k + 1])
        if starts.size == 0:
            continue
        cuts = np.flatnonzero(np.diff(starts) > k)  # a gap of more than k ends an interval
        first = np.concatenate(([0], cuts + 1))
        last = np.concatenate((cuts, [starts.size - 1]))
        for a, b in zip(first, last):
            out.append((e, int(starts[a]) - o, int(starts[b]) - o + k, int(b - a + 1)))
    return np.array(out, dtype=DTYPE).reshape(-1)
