"""Host-side mirror of the reference's per-contig polishing call.

The reference exposes its hot path as
    kmerizeAndCorrect(hdr, seq, len, bloom, bloomrep, dfout, rfout, vfout, clinvar)
(ntedit.cpp:1747) driven by readAndCorrect (ntedit.cpp:2154).  `Polisher`
keeps that shape: load the filter(s) once, set the opt:: parameters, then hand
it batches of contigs; it returns / writes `_edited.fa` and `_changes.tsv`.
All compute happens in libntedit_hip.so on the GPU.
"""
import ctypes
import numpy as np

from . import _lib
from ._lib import NtEditHipError, Params, Stats, Segment, WriteOptions, EDIT_DTYPE, QV_DTYPE, TRACK_DTYPE, DEPTH_DTYPE, APPLY_EDITED, APPLY_QV, APPLY_SHARED, APPLY_BGZF, APPLY_TRACK  # noqa: F401

PRIMARY, SECONDARY = 0, 1


def default_params(**kw):
    lib = _lib.load()
    p = Params()
    lib.ntedit_hip_params_default(ctypes.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def pack_batch(records, min_contig_len=0):
    """records: iterable of (header_bytes, sequence_bytes).  Returns the batch layout of
    include/ntedit_hip.h: (blob, offsets u64, lens u32, names) with one '\\n' behind every contig.
    Contigs shorter than min_contig_len are dropped (ntedit.cpp:2242)."""
    names, offs, lens, parts = [], [], [], []
    pos = 0
    for name, seq in records:
        if len(seq) < min_contig_len:
            continue
        names.append(bytes(name))
        offs.append(pos)
        lens.append(len(seq))
        parts.append(bytes(seq))
        parts.append(b"\n")
        pos += len(seq) + 1
    return b"".join(parts), np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32), names


class Result:
    def __init__(self, lib, handle, owner=None):
        self._lib, self._h = lib, handle
        self._owner = owner  # keeps the Polisher (and its context) alive as long as the result is

    def stats(self):
        s = Stats()
        self._lib.ntedit_hip_result_stats(self._h, ctypes.byref(s))
        return s

    @staticmethod
    def _blob_ptr(blob):
        """(keep-alive object, void*) of a host batch: numpy array (no copy), bytearray (no copy) or bytes"""
        if isinstance(blob, np.ndarray):
            buf = np.ascontiguousarray(blob, dtype=np.uint8)
            return buf, ctypes.c_void_p(buf.ctypes.data)
        if isinstance(blob, bytearray):
            arr = (ctypes.c_char * max(len(blob), 1)).from_buffer(blob)
            return arr, ctypes.cast(arr, ctypes.c_void_p)
        buf = blob if isinstance(blob, bytes) else bytes(blob)
        return buf, ctypes.cast(ctypes.c_char_p(buf), ctypes.c_void_p)

    @staticmethod
    def _segment_array(segments, n):
        """segments: None or a sequence of (pos_offset, halo, flags) per entry"""
        if segments is None:
            return None
        arr = (Segment * max(n, 1))()
        for i, (off, halo, flags) in enumerate(segments):
            arr[i].pos_offset, arr[i].halo, arr[i].flags = int(off), int(halo), int(flags)
        return arr

    def write(self, blob, offsets, lens, names, fa_path, tsv_path, append=False, vcf_path=None, snv=False, annot=None,
              segments=None, want_sizes=False):
        """Render the batch (ntedit_hip_write_outputs_ex).  SNV mode follows the parameters the batch was polished
        with (`snv` is ignored).  segments: per-entry (pos_offset, halo, flags) for contigs cut into segments.
        want_sizes: return an (n, 3) uint64 array with the bytes every entry appended to fa / tsv / vcf."""
        n = len(names)
        arr = (ctypes.c_char_p * max(n, 1))(*names)
        buf, ptr = self._blob_ptr(blob)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        seg = self._segment_array(segments, n)
        sizes = np.zeros((max(n, 1), 3), dtype=np.uint64) if want_sizes else None
        wo = WriteOptions()
        wo.fa_path = fa_path.encode() if fa_path else None
        wo.tsv_path = tsv_path.encode() if tsv_path else None
        wo.vcf_path = vcf_path.encode() if vcf_path else None
        wo.append = 1 if append else 0
        wo.annot = annot
        wo.segments = ctypes.cast(seg, ctypes.c_void_p) if seg is not None else None
        wo.out_sizes = sizes.ctypes.data if sizes is not None else None
        rc = self._lib.ntedit_hip_write_outputs_ex(
            self._h, ptr, offsets.ctypes.data_as(ctypes.c_void_p), lens.ctypes.data_as(ctypes.c_void_p), arr, n,
            ctypes.byref(wo))
        if rc:
            raise NtEditHipError("write_outputs failed (%d)%s" % (
                rc, ": a segment's cut is not event-free" if rc == _lib.E_SEGMENT else ""))
        return sizes[:n] if sizes is not None else None

    def cover_ends(self, n_contigs):
        """per entry: where the serial run of its last applied event ended (0 = no applied event)"""
        out = np.zeros(max(n_contigs, 1), dtype=np.uint32)
        rc = self._lib.ntedit_hip_result_cover_ends(self._h, n_contigs, out.ctypes.data_as(ctypes.c_void_p))
        if rc:
            raise NtEditHipError("result_cover_ends failed (%d)" % rc)
        return out[:n_contigs]

    def cuts_ok(self, lens, segments):
        """per entry: will write() accept it with this (pos_offset, halo, flags)?  The renderer's own predicate
        (ntedit_hip_result_cuts_ok); an entry that fails is polished again joined with its successor."""
        n = len(lens)
        seg = self._segment_array(segments, n)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        ok = np.zeros(max(n, 1), dtype=np.uint8)
        rc = self._lib.ntedit_hip_result_cuts_ok(self._h, n, lens.ctypes.data_as(ctypes.c_void_p),
                                                 ctypes.cast(seg, ctypes.c_void_p), ok.ctypes.data_as(ctypes.c_void_p))
        if rc:
            raise NtEditHipError("result_cuts_ok failed (%d)" % rc)
        return ok[:n].astype(bool)

    def edits(self, blob, offsets, lens, segments=None):
        """(records, pool): every _changes.tsv row as a numpy record (dtype _lib.EDIT_DTYPE) plus the byte pool
        the inserted / deleted bases live in"""
        n = len(lens)
        buf, ptr = self._blob_ptr(blob)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        seg = self._segment_array(segments, n)
        ed, cnt, pool = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p()
        rc = self._lib.ntedit_hip_result_edits(
            self._h, ptr, offsets.ctypes.data_as(ctypes.c_void_p), lens.ctypes.data_as(ctypes.c_void_p), n,
            ctypes.cast(seg, ctypes.c_void_p) if seg is not None else None, ctypes.byref(ed), ctypes.byref(cnt),
            ctypes.byref(pool))
        if rc:
            raise NtEditHipError("result_edits failed (%d)" % rc)
        dt = np.dtype(EDIT_DTYPE)
        if cnt.value == 0:
            return np.zeros(0, dtype=dt), b""
        recs = np.frombuffer(ctypes.string_at(ed.value, cnt.value * dt.itemsize), dtype=dt).copy()
        need = int((recs["bases_off"].astype(np.int64) + recs["len"]).max())
        return recs, ctypes.string_at(pool.value, need)

    def _result_error(self, what, rc):
        msg = self._lib.ntedit_hip_result_last_error()
        raise NtEditHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    def edited_device(self, n_contigs):
        """(device pointer, bytes, offsets u64, lens u32) of the edited contigs in HBM; needs set_apply(APPLY_EDITED)"""
        ptr, nb = ctypes.c_void_p(), ctypes.c_uint64()
        offs = np.zeros(max(n_contigs, 1), dtype=np.uint64)
        lens = np.zeros(max(n_contigs, 1), dtype=np.uint32)
        rc = self._lib.ntedit_hip_result_edited_device(self._h, ctypes.byref(ptr), ctypes.byref(nb),
                                                       offs.ctypes.data_as(ctypes.c_void_p),
                                                       lens.ctypes.data_as(ctypes.c_void_p), n_contigs)
        if rc:
            self._result_error("result_edited_device", rc)
        return ptr.value or 0, nb.value, offs[:n_contigs], lens[:n_contigs]

    def edited(self, n_contigs):
        """(bytes uint8, offsets u64, lens u32): the edited contigs, downloaded -- entry i is
        bytes[offsets[i] : offsets[i] + lens[i]], the sequence line of _edited.fa; needs set_apply(APPLY_EDITED)"""
        _, nb, offs, lens = self.edited_device(n_contigs)
        buf = np.zeros(max(nb, 1), dtype=np.uint8)
        need = ctypes.c_uint64()
        rc = self._lib.ntedit_hip_result_edited(self._h, buf.ctypes.data_as(ctypes.c_void_p), nb, ctypes.byref(need),
                                                None, None, n_contigs)
        if rc:
            self._result_error("result_edited", rc)
        return buf[:nb], offs, lens

    def qv(self, n_contigs):
        """one record per entry (dtype _lib.QV_DTYPE): lengths, k-mer starts and absent k-mers before and after;
        needs set_apply(APPLY_QV)"""
        rows = np.zeros(max(n_contigs, 1), dtype=np.dtype(QV_DTYPE))
        rc = self._lib.ntedit_hip_result_qv(self._h, rows.ctypes.data_as(ctypes.c_void_p), n_contigs)
        if rc:
            self._result_error("result_qv", rc)
        return rows[:n_contigs]

    def track(self, which):
        """the unsupported regions before (which = 0) or after (1) the polish, one record per interval (dtype
        _lib.TRACK_DTYPE: entry, begin, end, absent), ordered by entry, then begin; needs set_apply(APPLY_TRACK)"""
        n = ctypes.c_uint64()
        rc = self._lib.ntedit_hip_result_track(self._h, int(which), None, 0, ctypes.byref(n))
        if rc and rc != _lib.E_OVERFLOW:
            self._result_error("result_track", rc)
        recs = np.zeros(max(n.value, 1), dtype=np.dtype(TRACK_DTYPE))
        rc = self._lib.ntedit_hip_result_track(self._h, int(which), recs.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n))
        if rc:
            self._result_error("result_track", rc)
        return recs[:n.value]

    def spectrum(self, which):
        """uint64[256]: the k-mer occurrences at every multiplicity 0 .. 255 before (which = 0) or after (1) the polish,
        against the counting PRIMARY filter; needs set_spectrum(True)"""
        bins = np.zeros(256, dtype=np.uint64)
        rc = self._lib.ntedit_hip_result_spectrum(self._h, int(which), bins.ctypes.data_as(ctypes.c_void_p))
        if rc:
            self._result_error("result_spectrum", rc)
        return bins

    def depth(self, n_contigs):
        """one record per entry (dtype _lib.DEPTH_DTYPE): k-mer occurrences, the sum of their multiplicities and the
        saturated ones, before and after; needs set_spectrum(True)"""
        rows = np.zeros(max(n_contigs, 1), dtype=np.dtype(DEPTH_DTYPE))
        rc = self._lib.ntedit_hip_result_depth(self._h, rows.ctypes.data_as(ctypes.c_void_p), n_contigs)
        if rc:
            self._result_error("result_depth", rc)
        return rows[:n_contigs]

    def fa_bgzf(self):
        """(bytes, plain bytes, members): the batch's _edited.fa text as BGZF members, copied out of the result's
        page-locked buffer; needs set_apply(APPLY_BGZF) and set_fa_names() before the polish call"""
        ptr, nb, plain, members = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._lib.ntedit_hip_result_fa_bgzf(self._h, ctypes.byref(ptr), ctypes.byref(nb), ctypes.byref(plain),
                                                 ctypes.byref(members))
        if rc:
            self._result_error("result_fa_bgzf", rc)
        return (ctypes.string_at(ptr.value, nb.value) if nb.value else b""), plain.value, members.value

    def free(self):
        if self._h:
            self._lib.ntedit_hip_result_free(self._h)
            self._h = None

    def __del__(self):
        self.free()


class Polisher:
    def __init__(self, device=0):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self._lib.ntedit_hip_create(device, ctypes.byref(h))
        if rc:
            raise NtEditHipError("ntedit_hip_create(device=%d) failed (%d): no usable HIP device" % (device, rc))
        self._h = h
        self.params = default_params()

    def _check(self, rc, what):
        if rc:
            msg = self._lib.ntedit_hip_last_error(self._h)
            raise NtEditHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    def close(self):
        # results hold page-locked buffers that belong to the context: free them first
        if self._h:
            self._lib.ntedit_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- filters
    def load_filter_file(self, path, slot=PRIMARY):
        self._check(self._lib.ntedit_hip_load_filter_file(self._h, slot, path.encode()), "load_filter_file")

    def set_filter(self, bits, hash_num, k, slot=PRIMARY, counting=False):
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        self._check(self._lib.ntedit_hip_set_filter(self._h, slot, bits.ctypes.data_as(ctypes.c_void_p),
                                                    bits.size, hash_num, k, int(counting)), "set_filter")

    def set_filter_device(self, device_ptr, nbytes, hash_num, k, slot=PRIMARY, counting=False):
        self._check(self._lib.ntedit_hip_set_filter_device(self._h, slot, ctypes.c_void_p(device_ptr), nbytes,
                                                           hash_num, k, int(counting)), "set_filter_device")

    def filter_alloc(self, nbytes, hash_num, k, slot=PRIMARY):
        self._check(self._lib.ntedit_hip_filter_alloc(self._h, slot, nbytes, hash_num, k), "filter_alloc")

    def filter_insert(self, bases, slot=PRIMARY, device_ptr=None, n=None):
        if device_ptr is not None:
            rc = self._lib.ntedit_hip_filter_insert(self._h, slot, ctypes.c_void_p(device_ptr), n, 1)
        else:
            rc = self._lib.ntedit_hip_filter_insert(self._h, slot, ctypes.cast(ctypes.c_char_p(bases), ctypes.c_void_p),
                                                    len(bases), 0)
        self._check(rc, "filter_insert")

    def filter_download(self, slot=PRIMARY):
        k, h, nb, cnt = self.filter_info(slot)
        out = np.empty(nb, dtype=np.uint8)
        self._check(self._lib.ntedit_hip_filter_download(self._h, slot, out.ctypes.data_as(ctypes.c_void_p)),
                    "filter_download")
        return out

    def filter_occupancy(self, slot=PRIMARY):
        """(occupied, slots): set bits / non-zero counters and the filter's size in slots"""
        occ, slots = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.ntedit_hip_filter_occupancy(self._h, slot, ctypes.byref(occ), ctypes.byref(slots)),
                    "filter_occupancy")
        return occ.value, slots.value

    def filter_save_file(self, path, slot=PRIMARY):
        self._check(self._lib.ntedit_hip_filter_save_file(self._h, slot, path.encode()), "filter_save_file")

    def filter_info(self, slot=PRIMARY):
        k, h, nb, cnt = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_int()
        self._check(self._lib.ntedit_hip_filter_info(self._h, slot, ctypes.byref(k), ctypes.byref(h),
                                                     ctypes.byref(nb), ctypes.byref(cnt)), "filter_info")
        return k.value, h.value, nb.value, bool(cnt.value)

    def filter_device_ptr(self, slot=PRIMARY):
        return self._lib.ntedit_hip_filter_device_ptr(self._h, slot)

    # ---- parameters
    def set_params(self, params):
        self.params = params
        self._check(self._lib.ntedit_hip_set_params(self._h, ctypes.byref(params)), "set_params")

    # ---- hot path
    def screen(self, blob):
        """absent bitmap (np.uint64 words) for a host batch"""
        n = len(blob)
        out = np.zeros((n + 63) // 64, dtype=np.uint64)
        self._check(self._lib.ntedit_hip_screen(self._h, ctypes.cast(ctypes.c_char_p(blob), ctypes.c_void_p), n, 0,
                                                out.ctypes.data_as(ctypes.c_void_p)), "screen")
        return out

    def screen_device(self, bases_ptr, n, bitmap_ptr):
        self._check(self._lib.ntedit_hip_screen(self._h, ctypes.c_void_p(bases_ptr), n, 1,
                                                ctypes.c_void_p(bitmap_ptr)), "screen")
        return self._lib.ntedit_hip_last_kernel_ms(self._h)

    def pack_bases(self, blob, out=None, threads=0):
        """The packed form of a host batch (4-bit codes + case bits, include/ntedit_hip.h), or None when the batch holds a
        byte that form cannot carry.  out: a uint8 buffer of packed_size(len(blob)) bytes (e.g. page-locked)."""
        n = len(blob)
        size = int(self._lib.ntedit_hip_packed_size(n))
        if out is None:
            out = np.empty(size, dtype=np.uint8)
        assert out.nbytes >= size
        keep, ptr = Result._blob_ptr(blob)
        rc = self._lib.ntedit_hip_pack_bases(ptr, n, out.ctypes.data_as(ctypes.c_void_p), threads)
        del keep
        if rc < 0:
            raise NtEditHipError("pack_bases failed (%d)" % rc)
        return None if rc else out

    def packed_size(self, n):
        return int(self._lib.ntedit_hip_packed_size(n))

    def polish_batch(self, blob, offsets, lens, device_ptr=None, n=None, packed=None):
        """packed: the batch's packed form (pack_bases); it crosses PCIe instead of `blob`, whose length is still the batch's"""
        res = ctypes.c_void_p()
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        if packed is not None:
            rc = self._lib.ntedit_hip_polish_batch(self._h, packed.ctypes.data_as(ctypes.c_void_p), len(blob),
                                                   offsets.ctypes.data_as(ctypes.c_void_p),
                                                   lens.ctypes.data_as(ctypes.c_void_p), len(lens), 2,
                                                   ctypes.byref(res))
        elif device_ptr is not None:
            rc = self._lib.ntedit_hip_polish_batch(self._h, ctypes.c_void_p(device_ptr), n,
                                                   offsets.ctypes.data_as(ctypes.c_void_p),
                                                   lens.ctypes.data_as(ctypes.c_void_p), len(lens), 1,
                                                   ctypes.byref(res))
        else:
            keep, ptr = Result._blob_ptr(blob)  # bytes, bytearray or a numpy array (e.g. a page-locked buffer)
            rc = self._lib.ntedit_hip_polish_batch(self._h, ptr, len(blob), offsets.ctypes.data_as(ctypes.c_void_p),
                                                   lens.ctypes.data_as(ctypes.c_void_p), len(lens), 0,
                                                   ctypes.byref(res))
            del keep
        self._check(rc, "polish_batch")
        return Result(self._lib, res, self)

    def write_tsv_header(self, tsv_path):
        """header line of _changes.tsv for the loaded primary filter / current parameters"""
        k, _, _, counting = self.filter_info(PRIMARY)
        rc = self._lib.ntedit_hip_write_tsv_header(tsv_path.encode(), k, self.params.jump, int(counting))
        if rc:
            raise NtEditHipError("cannot write %s" % tsv_path)

    def set_apply(self, flags):
        """ntedit_hip_set_apply: 0, APPLY_EDITED (the result keeps the edited contigs in HBM: Result.edited()),
        APPLY_QV (k-mer counts before and after: Result.qv()), APPLY_SHARED (what APPLY_QV runs, and the present k-mers
        of the batch and of the edited bases marked for the completeness: shared_counts()), APPLY_BGZF (the batch's
        _edited.fa text compressed on the device: set_fa_names(), Result.fa_bgzf()), APPLY_TRACK (what APPLY_QV runs, and
        the unsupported regions before and after as intervals: Result.track()) or any of them together, for the
        polish_batch calls that follow"""
        self._check(self._lib.ntedit_hip_set_apply(self._h, int(flags)), "set_apply")

    def set_fa_names(self, names):
        """the header lines (bytes, without '>') of the entries of the NEXT polish_batch call: APPLY_BGZF needs them"""
        arr = (ctypes.c_char_p * max(len(names), 1))(*[bytes(n) for n in names])
        self._check(self._lib.ntedit_hip_set_fa_names(self._h, arr, len(names)), "set_fa_names")

    def bgzf_deflate(self, data=None, device_ptr=None, n=None):
        """bytes (or n device bytes at device_ptr) as BGZF members without the EOF member (ntedit_hip_bgzf_deflate)"""
        if device_ptr is not None:
            ptr, on_device = ctypes.c_void_p(device_ptr), 1
        else:
            keep, ptr = Result._blob_ptr(data)
            n, on_device = len(data), 0
        cap = int(self._lib.ntedit_hip_bgzf_bound(n))
        out = ctypes.create_string_buffer(max(cap, 1))
        need = ctypes.c_uint64()
        self._check(self._lib.ntedit_hip_bgzf_deflate(self._h, ptr, n, on_device, out, cap, ctypes.byref(need)),
                    "bgzf_deflate")
        return out.raw[:need.value]

    def bgzf_info(self):
        """ntedit_hip_bgzf_info of the last call that compressed: _lib.BgzfStats"""
        st = _lib.BgzfStats()
        self._check(self._lib.ntedit_hip_bgzf_info(self._h, ctypes.byref(st)), "bgzf_info")
        return st

    def apply_info(self):
        """ntedit_hip_apply_info of the last polish_batch: _lib.ApplyStats"""
        st = _lib.ApplyStats()
        self._check(self._lib.ntedit_hip_apply_info(self._h, ctypes.byref(st)), "apply_info")
        return st

    def qv_value(self, absent, kmers, k=None):
        if k is None:
            k = self.filter_info(PRIMARY)[0]
        return self._lib.ntedit_hip_qv_value(int(absent), int(kmers), int(k))

    def write_qv_table(self, path, names, rows, k=None):
        """<prefix>_qv.tsv: the header, one line per entry, the "#total" row (ntedit_hip_qv_format_row)"""
        if k is None:
            k = self.filter_info(PRIMARY)[0]
        buf = ctypes.create_string_buffer(1 << 16)
        total = _lib.QvRow()
        with open(path, "wb") as f:
            f.write(self._lib.ntedit_hip_qv_header())
            for name, r in zip(names, rows):
                row = _lib.QvRow(*[int(r[fld]) for fld, _ in _lib.QvRow._fields_])
                for fld, _ in _lib.QvRow._fields_:
                    setattr(total, fld, getattr(total, fld) + getattr(row, fld))
                if self._lib.ntedit_hip_qv_format_row(bytes(name), ctypes.byref(row), k, buf, len(buf)):
                    raise NtEditHipError("qv row of %r does not fit" % name)
                f.write(buf.value)
            self._lib.ntedit_hip_qv_format_row(b"#total", ctypes.byref(total), k, buf, len(buf))
            f.write(buf.value)
        return total

    # ---- the unsupported regions as intervals (nte_track.hip)
    def track_extract(self, bitmap, offs, lens, k, n=None):
        """the intervals of any absent bitmap (uint64 words, position p = bit p % 64 of word p / 64) over the entries
        offs / lens of a batch of n positions (default: 64 * len(bitmap)): records of dtype _lib.TRACK_DTYPE
        (ntedit_hip_track_extract)"""
        bitmap = np.ascontiguousarray(bitmap, dtype=np.uint64)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if len(a) else None  # noqa: E731
        n = 64 * len(bitmap) if n is None else int(n)
        if n > 64 * len(bitmap):
            raise NtEditHipError("track_extract: %d positions need more than %d bitmap words" % (n, len(bitmap)))
        args = (self._h, ptr(bitmap), n, ptr(offs), ptr(lens), len(offs), int(k))
        found = ctypes.c_uint64()
        rc = self._lib.ntedit_hip_track_extract(*args, None, 0, ctypes.byref(found))
        if rc != _lib.E_OVERFLOW:
            self._check(rc, "track_extract")
        recs = np.zeros(max(found.value, 1), dtype=np.dtype(TRACK_DTYPE))
        if found.value:
            self._check(self._lib.ntedit_hip_track_extract(*args, recs.ctypes.data_as(ctypes.c_void_p), found.value,
                                                           ctypes.byref(found)), "track_extract")
        return recs[:found.value]

    def track_info(self):
        """ntedit_hip_track_info of the last call that extracted intervals: _lib.TrackStats"""
        st = _lib.TrackStats()
        self._check(self._lib.ntedit_hip_track_info(self._h, ctypes.byref(st)), "track_info")
        return st

    def write_track_bed(self, path, names, intervals):
        """a four-column BED file without a header: name (cut at its first space or tab), begin, end, absent k-mers of
        every interval, in the intervals' order (ntedit_hip_track_format_row); returns the bases they cover"""
        buf = ctypes.create_string_buffer(1 << 16)
        covered = 0
        with open(path, "wb") as f:
            for r in intervals:
                iv = _lib.TrackInterval(int(r["entry"]), int(r["begin"]), int(r["end"]), int(r["absent"]))
                if self._lib.ntedit_hip_track_format_row(bytes(names[iv.entry]), ctypes.byref(iv), buf, len(buf)):
                    raise NtEditHipError("bed row of %r does not fit" % names[iv.entry])
                f.write(buf.value)
                covered += iv.end - iv.begin
        return covered

    # ---- the k-mer multiplicity spectrum against a counting PRIMARY filter (k_spectrum)
    def set_spectrum(self, on):
        """ntedit_hip_set_spectrum: the polish_batch calls that follow count the spectrum before and after
        (Result.spectrum(), Result.depth()); a switch of its own beside set_apply's flags"""
        self._check(self._lib.ntedit_hip_set_spectrum(self._h, int(bool(on))), "set_spectrum")

    def spectrum_count(self, blob, offs, lens, device_ptr=None, n=None, rows=True):
        """(bins uint64[256], rows of dtype _lib.SPECTRUM_ROW_DTYPE or None) of any batch -- host bytes, or n device
        bytes at device_ptr -- over the entries offs / lens (ntedit_hip_spectrum_count)"""
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if len(a) else None  # noqa: E731
        bins = np.zeros(256, dtype=np.uint64)
        out = np.zeros(max(len(offs), 1), dtype=np.dtype(_lib.SPECTRUM_ROW_DTYPE)) if rows else None
        if device_ptr is not None:
            keep, bases, n, on_device = None, ctypes.c_void_p(device_ptr), int(n), 1
        else:
            keep, bases = Result._blob_ptr(blob)
            n, on_device = len(blob), 0
        rc = self._lib.ntedit_hip_spectrum_count(self._h, bases, n, on_device, ptr(offs), ptr(lens), len(offs),
                                                 bins.ctypes.data_as(ctypes.c_void_p), ptr(out) if rows else None)
        del keep
        self._check(rc, "spectrum_count")
        return bins, (out[:len(offs)] if rows else None)

    def spectrum_info(self):
        """ntedit_hip_spectrum_info of the last call that counted a spectrum: _lib.SpectrumStats"""
        st = _lib.SpectrumStats()
        self._check(self._lib.ntedit_hip_spectrum_info(self._h, ctypes.byref(st)), "spectrum_info")
        return st

    def write_spectrum_tables(self, out_prefix, names, bins_before, bins_after, depth):
        """<prefix>_spectrum.tsv (the header, 256 rows) and <prefix>_depth.tsv (the header, one row per entry, "#total"),
        through the library's formatters"""
        buf = ctypes.create_string_buffer(1 << 16)
        with open(out_prefix + "_spectrum.tsv", "wb") as f:
            f.write(self._lib.ntedit_hip_spectrum_header())
            for c in range(256):
                self._lib.ntedit_hip_spectrum_format_row(c, int(bins_before[c]), int(bins_after[c]), buf, len(buf))
                f.write(buf.value)
        total = _lib.DepthRow()
        with open(out_prefix + "_depth.tsv", "wb") as f:
            f.write(self._lib.ntedit_hip_depth_header())
            for name, r in zip(names, depth):
                row = _lib.DepthRow(*[int(r[fld]) for fld, _ in _lib.DepthRow._fields_])
                for fld, _ in _lib.DepthRow._fields_:
                    setattr(total, fld, getattr(total, fld) + getattr(row, fld))
                if self._lib.ntedit_hip_depth_format_row(bytes(name), ctypes.byref(row), buf, len(buf)):
                    raise NtEditHipError("depth row of %r does not fit" % name)
                f.write(buf.value)
            self._lib.ntedit_hip_depth_format_row(b"#total", ctypes.byref(total), buf, len(buf))
            f.write(buf.value)
        return total

    # ---- the spectrum split by assembly copy number (nte_cn.hip)
    def set_cn(self, on, store_cap_bytes=_lib.CN_STORE_DEFAULT):
        """ntedit_hip_set_cn: the polish_batch calls that follow append the batch and its edited entries to the draft
        store in HBM (at most store_cap_bytes of bases); cn_finish() then counts both sides"""
        self._check(self._lib.ntedit_hip_set_cn(self._h, int(bool(on)), int(store_cap_bytes)), "set_cn")

    def cn_append(self, which, blob, offs, lens, device_ptr=None, n=None):
        """one batch -- host bytes, or n device bytes at device_ptr -- to side `which` (0 before, 1 after) of the store"""
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if len(a) else None  # noqa: E731
        if device_ptr is not None:
            keep, bases, n, on_device = None, ctypes.c_void_p(device_ptr), int(n), 1
        else:
            keep, bases = Result._blob_ptr(blob)
            n, on_device = len(blob), 0
        rc = self._lib.ntedit_hip_cn_append(self._h, int(which), bases, n, on_device, ptr(offs), ptr(lens), len(offs))
        del keep
        self._check(rc, "cn_append")

    def cn_finish(self, sketch_counters=0):
        """ntedit_hip_cn_finish: both sides counted from the store; sketch_counters 0 picks the size"""
        self._check(self._lib.ntedit_hip_cn_finish(self._h, int(sketch_counters)), "cn_finish")

    def cn_table(self, which):
        """(occ uint64[5][256], w5 uint64[256]) of one side: occurrences by class (copy number 1, 2, 3, 4, 5 or more) and
        multiplicity, and the class-5 weights"""
        occ = np.zeros((5, 256), dtype=np.uint64)
        w5 = np.zeros(256, dtype=np.uint64)
        rc = self._lib.ntedit_hip_cn_table(self._h, int(which), occ.ctypes.data_as(ctypes.c_void_p), w5.ctypes.data_as(ctypes.c_void_p))
        self._check(rc, "cn_table")
        return occ, w5

    def cn_rows(self, which, n):
        """one record per entry of side `which` in the order appended (dtype _lib.CN_ROW_DTYPE)"""
        rows = np.zeros(max(n, 1), dtype=np.dtype(_lib.CN_ROW_DTYPE))
        self._check(self._lib.ntedit_hip_cn_rows(self._h, int(which), rows.ctypes.data_as(ctypes.c_void_p), int(n)), "cn_rows")
        return rows[:n]

    def cn_distinct(self, occ, w5):
        """uint64[5][256] distinct k-mers from a side's table (host only)"""
        occ = np.ascontiguousarray(occ, dtype=np.uint64)
        w5 = np.ascontiguousarray(w5, dtype=np.uint64)
        out = np.zeros((5, 256), dtype=np.uint64)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        if self._lib.ntedit_hip_cn_distinct(ptr(occ), ptr(w5), ptr(out)):
            raise NtEditHipError("cn_distinct: bad argument")
        return out

    def cn_info(self):
        """ntedit_hip_cn_info: _lib.CnStats"""
        st = _lib.CnStats()
        self._check(self._lib.ntedit_hip_cn_info(self._h, ctypes.byref(st)), "cn_info")
        return st

    def cn_reset(self):
        self._check(self._lib.ntedit_hip_cn_reset(self._h), "cn_reset")

    def cn_free(self):
        self._check(self._lib.ntedit_hip_cn_free(self._h), "cn_free")

    def write_cn_tables(self, out_prefix, names, distinct_before, distinct_after, rows_before, rows_after):
        """<prefix>_spectrum_cn.tsv (the header, 256 rows of distinct k-mers) and <prefix>_cn_contigs.tsv (the header, one
        row per entry, "#total"), through the library's formatters; returns the two total rows"""
        buf = ctypes.create_string_buffer(1 << 16)
        d0 = np.ascontiguousarray(distinct_before, dtype=np.uint64)
        d1 = np.ascontiguousarray(distinct_after, dtype=np.uint64)
        with open(out_prefix + "_spectrum_cn.tsv", "wb") as f:
            f.write(self._lib.ntedit_hip_cn_header())
            for m in range(256):
                self._lib.ntedit_hip_cn_format_row(m, d0.ctypes.data_as(ctypes.c_void_p), d1.ctypes.data_as(ctypes.c_void_p), buf, len(buf))
                f.write(buf.value)
        total = _lib.CnRow(), _lib.CnRow()
        with open(out_prefix + "_cn_contigs.tsv", "wb") as f:
            f.write(self._lib.ntedit_hip_cn_contig_header())
            for name, rb, ra in zip(names, rows_before, rows_after):
                pair = [_lib.CnRow(*[int(r[fld]) for fld, _ in _lib.CnRow._fields_]) for r in (rb, ra)]
                for t, row in zip(total, pair):
                    for fld, _ in _lib.CnRow._fields_:
                        setattr(t, fld, getattr(t, fld) + getattr(row, fld))
                if self._lib.ntedit_hip_cn_contig_format_row(bytes(name), ctypes.byref(pair[0]), ctypes.byref(pair[1]), buf, len(buf)):
                    raise NtEditHipError("cn row of %r does not fit" % name)
                f.write(buf.value)
            self._lib.ntedit_hip_cn_contig_format_row(b"#total", ctypes.byref(total[0]), ctypes.byref(total[1]), buf, len(buf))
            f.write(buf.value)
        return total

    # ---- k-mer completeness: the draft's distinct k-mers that the PRIMARY filter holds
    def shared_begin(self):
        """allocate and zero the two mark arrays (before, after) for the current PRIMARY filter; idempotent"""
        self._check(self._lib.ntedit_hip_shared_begin(self._h), "shared_begin")

    def shared_reset(self):
        self._check(self._lib.ntedit_hip_shared_reset(self._h), "shared_reset")

    def shared_free(self):
        self._lib.ntedit_hip_shared_free(self._h)

    def shared_mark(self, blob, which=0):
        """screen a host batch (entries + separators) with -s 0 semantics and mark its present k-mers into array `which`"""
        self._check(self._lib.ntedit_hip_shared_mark(self._h, int(which), ctypes.cast(ctypes.c_char_p(blob), ctypes.c_void_p),
                                                     len(blob), 0), "shared_mark")

    def shared_download(self, which=0):
        """mark array `which` as uint8 bytes of the PRIMARY filter's size"""
        nb = self.filter_info(PRIMARY)[2]
        out = np.empty(nb, dtype=np.uint8)
        self._check(self._lib.ntedit_hip_shared_download(self._h, int(which), out.ctypes.data_as(ctypes.c_void_p)),
                    "shared_download")
        return out

    def shared_counts(self):
        """ntedit_hip_shared_counts: _lib.SharedStats (the popcounts of the filter and of both mark arrays)"""
        st = _lib.SharedStats()
        self._check(self._lib.ntedit_hip_shared_counts(self._h, ctypes.byref(st)), "shared_counts")
        return st

    def bloom_cardinality(self, set_bits, slots, h=1):
        return self._lib.ntedit_hip_bloom_cardinality(int(set_bits), int(slots), int(h))

    def polish_records(self, records, out_prefix, draft_name="", annot_path=None, qv=False, bed=False, spectrum=False):
        """readAndCorrect at -t 1 for an in-memory list of (header, sequence): writes
        <prefix>_edited.fa, <prefix>_changes.tsv and <prefix>_variants.vcf; returns Stats.
        qv: also <prefix>_qv.tsv, the k-mer QV of every contig before and after (set_apply(APPLY_QV) for this call).
        bed: also <prefix>_absent_before.bed (the draft's coordinates) and <prefix>_absent_after.bed (those of
        _edited.fa), the regions the filter does not support (set_apply(APPLY_TRACK) for this call).
        spectrum: also <prefix>_spectrum.tsv and <prefix>_depth.tsv, the k-mer multiplicity spectrum and the depth of every
        contig before and after, against a counting PRIMARY filter (set_spectrum(True) for this call)."""
        blob, offs, lens, names = pack_batch(records, self.params.min_contig_len)
        tsv = out_prefix + "_changes.tsv"
        fa = out_prefix + "_edited.fa"
        vcf = out_prefix + "_variants.vcf"
        self.write_tsv_header(tsv)
        self._lib.ntedit_hip_write_vcf_header(vcf.encode(), draft_name.encode())
        open(fa, "wb").close()
        annot = ctypes.c_void_p()
        if annot_path:
            if self._lib.ntedit_hip_annot_load(annot_path.encode(), ctypes.byref(annot)):
                raise NtEditHipError("cannot read %s" % annot_path)
        # (send_packed: the batch crosses PCIe as 4-bit codes + case bits when it can; the renderer keeps the bytes)
        packed = self.pack_bases(blob) if getattr(self, "send_packed", False) and len(blob) else None
        if qv or bed:
            self.set_apply((APPLY_QV if qv else 0) | (APPLY_TRACK if bed else 0))
        if spectrum:
            self.set_spectrum(True)
        try:
            res = self.polish_batch(blob, offs, lens, packed=packed)
        finally:
            if qv or bed:
                self.set_apply(0)
            if spectrum:
                self.set_spectrum(False)
        res.write(blob, offs, lens, names, fa, tsv, append=True, vcf_path=vcf, snv=bool(self.params.snv), annot=annot)
        if qv:
            self.write_qv_table(out_prefix + "_qv.tsv", names, res.qv(len(names)))
        if bed:
            for which, stage in enumerate(("before", "after")):
                self.write_track_bed("%s_absent_%s.bed" % (out_prefix, stage), names, res.track(which))
        if spectrum:
            self.write_spectrum_tables(out_prefix, names, res.spectrum(0), res.spectrum(1), res.depth(len(names)))
        if annot_path:
            self._lib.ntedit_hip_annot_free(annot)
        st = res.stats()
        res.free()
        return st

    def reserve(self, max_batch_bytes, max_contigs=0, events_hint=0, on_device=0):
        """ntedit_hip_reserve: buffers for batches of up to max_batch_bytes + one internal warm-up batch, so that the
        first polish_batch of this context costs what a warm one does (on_device: 0 host, 1 device, 2 packed batches)"""
        self._check(self._lib.ntedit_hip_reserve(self._h, int(max_batch_bytes), int(max_contigs), int(events_hint),
                                                 int(on_device)), "reserve")

    def device_tables(self):
        """ntedit_hip_device_tables: the reference's candidate tables as the device code holds them, as text"""
        buf = ctypes.create_string_buffer(1 << 16)
        n = ctypes.c_uint64()
        self._check(self._lib.ntedit_hip_device_tables(self._h, buf, ctypes.c_uint64(len(buf)), ctypes.byref(n)), "device_tables")
        return buf.raw[:n.value].decode()

    def settle_info(self):
        """ntedit_hip_settle_info: (events seen, events settled, ms) of k_settle in the last polish_batch"""
        st = _lib.SettleStats()
        self._check(self._lib.ntedit_hip_settle_info(self._h, ctypes.byref(st)), "settle_info")
        return st.events_seen, st.events_settled, st.ms

    def set_tuning(self, key, value):
        """Test / tuning knobs (include/ntedit_hip.h: none of them can change a result)."""
        self._check(self._lib.ntedit_hip_set_tuning(self._h, key.encode(), int(value)), "set_tuning")

    def gather_bench(self, nbytes, n_probes):
        pps, ms = ctypes.c_double(), ctypes.c_float()
        self._check(self._lib.ntedit_hip_gather_bench(self._h, nbytes, n_probes, ctypes.byref(pps), ctypes.byref(ms)),
                    "gather_bench")
        return pps.value, ms.value
