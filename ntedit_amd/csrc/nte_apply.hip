// nte_apply.hip -- the device applier (a result's arena -> the edited contigs in HBM) and the k-mer QV counts.
// Stages and data: nte_apply.h.  The specification of the applier is host/render.cpp (render_contig and the FASTA part
// of write_contig); every rule below names the line of thought it restates.
#include "nte_apply.h"
#include "nte_tile.h" // (entry_behind, bit_range)

namespace nte {

namespace {

struct ANode
{
	int type; // 0 position node, 1 inserted base, -1 end of the rope
	u32 c, s, e;
};

__device__ __forceinline__ Item
load_item(const Item* p)
{
	const uint4 v = *reinterpret_cast<const uint4*>(p);
	Item it;
	it.w[0] = v.x;
	it.w[1] = v.y;
	it.w[2] = v.z;
	it.w[3] = v.w;
	return it;
}

__device__ __forceinline__ ANode
node_of(const Item& it)
{
	ANode n;
	n.type = (int)(int8_t)((it.w[0] >> 8) & 0xFF);
	n.c = (it.w[0] >> 16) & 0xFF;
	n.s = it.w[1];
	n.e = it.w[2];
	return n;
}

__device__ __forceinline__ u32
pack_node(const ANode& n)
{
	return ((u32)n.type & 0xFF) | (n.c << 8);
}

// bytes a node emits (write_contig: type 0 seq[s_pos .. e_pos], type 1 its byte, anything else nothing); a position node
// must lie inside its contig -- s_pos == e_pos + 1 is the empty node
__device__ __forceinline__ u32
node_len(int type, u32 s, u32 e, u32 len, u32& err)
{
	if (type == 0) {
		if (e >= len || s > e + 1) {
			err |= AP_BAD_ITEM;
			return 0;
		}
		return e + 1 - s;
	}
	return type == 1 ? 1u : 0u;
}

// the items of an event's chunk chain, in order (render_contig's walk: the first chunk holds the link and the header in
// front of them); f returns false to stop.  Every index is checked against the arena, the chain is at most as long as the
// arena has chunks.
template<class F>
__device__ __forceinline__ u32
walk_event(const Item* __restrict__ arena, u64 arena_items, u32 fc, F&& f)
{
	const u64 max_chunks = arena_items / CHUNK_ITEMS;
	u64 steps = 0;
	u32 chunk = fc;
	bool first = true;
	while (chunk != NONE32) {
		if (((u64)chunk + 1) * CHUNK_ITEMS > arena_items || ++steps > max_chunks) {
			return AP_BAD_INDEX;
		}
		const Item* c = arena + (u64)chunk * CHUNK_ITEMS;
		const Item link = load_item(c);
		const u32 next = link.w[0], cnt = link.w[1];
		if (cnt > CHUNK_ITEMS) {
			return AP_BAD_COUNT;
		}
		for (u32 i = first ? 2 : 1; i < cnt; i++) {
			const Item it = load_item(c + i);
			const u32 tag = it.w[0] & 0xFF;
			if (tag != TAG_NODE && tag != TAG_SUB && tag != TAG_MOD) {
				return AP_BAD_ITEM;
			}
			if (!f(it, tag)) {
				return 0;
			}
		}
		first = false;
		chunk = next;
	}
	return 0;
}

// ---------------------------------------------------------------------------------------------- k_apply_summary
__global__ __launch_bounds__(APPLY_TPB) void
k_apply_summary(ApplyArgs a)
{
	const u32 i = blockIdx.x * APPLY_TPB + threadIdx.x;
	const u32 lane = threadIdx.x & 63;
	ApplyEvent ev;
	ev.start = ev.cover_end = ev.hflags = 0;
	ev.contig = NONE32;
	ev.n_nodes = 0;
	ev.first = ev.first_s = ev.first_e = ev.last = ev.last_s = ev.last_e = ev.mid_len = 0;
	u32 err = 0;
	const u32 fc = i < a.n_events ? a.ev_first[i] : NONE32;
	if (fc != NONE32) {
		if ((u64)fc * CHUNK_ITEMS + 1 >= a.arena_items) {
			err = AP_BAD_INDEX;
		} else {
			const Item h = load_item(a.arena + (u64)fc * CHUNK_ITEMS + 1);
			if (h.w[0] >= a.n_contigs) {
				err = AP_BAD_ORDER;
			} else {
				ev.contig = h.w[0];
				ev.start = h.w[1];
				ev.cover_end = h.w[2];
				ev.hflags = h.w[3];
			}
		}
	}
	if (ev.contig != NONE32 && !(ev.hflags & EV_UNFINISHED)) { // (what a parked event emitted is void)
		const u32 len = a.lens[ev.contig];
		ANode first, last;
		first.type = last.type = 0;
		first.c = first.s = first.e = last.c = last.s = last.e = 0;
		u32 n = 0, mid = 0;
		err |= walk_event(a.arena, a.arena_items, fc, [&](const Item& it, u32 tag) {
			if (tag != TAG_NODE) {
				return true;
			}
			const ANode nd = node_of(it);
			if (n == 0) {
				first = nd;
			} else {
				if (n >= 2) {
					mid += node_len(last.type, last.s, last.e, len, err);
				}
				// (only the first node may inherit its s_pos: every other one is checked as it stands)
				u32 e2 = 0;
				(void)node_len(nd.type, nd.s, nd.e, len, e2);
				err |= e2;
			}
			last = nd;
			n++;
			return nd.type != -1; // the rope ends here: later nodes are ignored
		});
		ev.n_nodes = n;
		ev.first = pack_node(first);
		ev.first_s = first.s;
		ev.first_e = first.e;
		ev.last = pack_node(last);
		ev.last_s = last.s;
		ev.last_e = last.e;
		ev.mid_len = mid;
	}
	if (i < a.n_events) {
		a.ev[i] = ev;
	}
	// the contigs' event ranges: one atomic where the contig changes inside the wavefront
	const u32 prev = __shfl_up(ev.contig, 1);
	const u32 next = __shfl_down(ev.contig, 1);
	if (ev.contig != NONE32) {
		if (lane == 0 || prev != ev.contig) {
			atomicMin(a.ev_begin + ev.contig, i);
		}
		if (lane == 63 || next != ev.contig) {
			atomicMax(a.ev_end + ev.contig, i + 1);
		}
	}
	if (err) {
		atomicOr(a.status, err);
	}
}

// ------------------------------------------------------------------------------------------------ k_apply_chain
// One wavefront per contig.  The serial order (render_contig: an event is applied iff start >= cover, then cover =
// cover_end) is resolved 64 events at a time: every lane holds one event, the next applied one is the first lane at or
// behind the cursor whose start reaches the cover -- a ballot and a find-first-set --, its fields come over by shuffle.
// The same walk carries the open node (the node that ends the rope: an applied event's first node replaces it and
// inherits its s_pos when its own type and s_pos are 0), the bytes and the pieces in front of every applied event.
__global__ __launch_bounds__(APPLY_TPB) void
k_apply_chain(ApplyArgs a)
{
	const u32 lane = threadIdx.x & 63;
	const u32 ci = blockIdx.x * (APPLY_TPB / 64) + (threadIdx.x >> 6);
	if (ci >= a.n_contigs) {
		return;
	}
	const u32 len = a.lens[ci];
	u32 b = a.ev_begin[ci], e = a.ev_end[ci];
	if (b == NONE32 || e <= b) {
		b = e = 0;
	}
	u32 cover = 0, err = 0;
	int open_type = 0;
	u32 open_c = 0, open_s = 0, open_e = len ? len - 1 : 0;
	bool term = false;
	u64 out = 0;
	u32 pieces = 0, applied = 0;
	for (u32 base = b; base < e && !err; base += 64) {
		const u32 idx = base + lane;
		ApplyEvent me;
		me.contig = NONE32;
		me.start = 0;
		if (idx < e) {
			me = a.ev[idx];
		}
		const bool valid = idx < e && me.contig == ci;
		u32 cur = 0;
		while (true) {
			const u64 m = __ballot(valid && lane >= cur && me.start >= cover);
			if (!m) {
				break;
			}
			const u32 j = (u32)__ffsll((unsigned long long)m) - 1;
			cur = j + 1;
			const u32 hflags = __shfl(me.hflags, j);
			if (hflags & EV_UNFINISHED) {
				err |= AP_UNFINISHED; // a parked event must have been re-run before it can be applied
				break;
			}
			cover = __shfl(me.cover_end, j);
			applied++;
			const u32 n_nodes = __shfl(me.n_nodes, j);
			ApplyPlace pl;
			pl.out_off = (u32)out;
			pl.piece = pieces;
			pl.open_s = open_s;
			pl.flags = 1;
			if (n_nodes && !term) {
				pl.flags |= 2;
				const u32 first = __shfl(me.first, j);
				const int ftype = (int)(int8_t)(first & 0xFF);
				u32 fs = __shfl(me.first_s, j);
				const u32 fe = __shfl(me.first_e, j);
				if (ftype == 0 && fs == 0) {
					fs = open_s;
				}
				if (n_nodes == 1) {
					open_type = ftype;
					open_c = first >> 8;
					open_s = fs;
					open_e = fe;
				} else {
					out += (u64)node_len(ftype, fs, fe, len, err) + __shfl(me.mid_len, j);
					pieces += n_nodes - 1;
					const u32 last = __shfl(me.last, j);
					open_type = (int)(int8_t)(last & 0xFF);
					open_c = last >> 8;
					open_s = __shfl(me.last_s, j);
					open_e = __shfl(me.last_e, j);
				}
				term = open_type == -1;
			}
			if (lane == j) {
				a.place[idx] = pl;
			}
			if (out > 0xFFFFFFFFull) {
				err |= AP_TOO_LONG;
				break;
			}
		}
		// (events the serial order skipped keep the flags 0 the buffer was cleared to)
	}
	const u32 olen = len ? node_len(open_type, open_s, open_e, len, err) : 0;
	if (out + olen > 0xFFFFFFFFull) {
		err |= AP_TOO_LONG;
	}
	if (lane == 0) {
		ApplyContig c;
		c.out_len = err ? 0 : out + olen;
		c.n_pieces = pieces + 2;
		c.open = ((u32)open_type & 0xFF) | (open_c << 8);
		c.open_s = open_s;
		c.open_e = len ? open_e : 0;
		c.open_off = (u32)out;
		c.applied = applied;
		a.contig[ci] = c;
		if (err) {
			atomicOr(a.status, err);
		}
	}
}

// ------------------------------------------------------------------------------------------------- k_apply_scan
// 64-bit exclusive scans over the contigs: output bytes (one separator byte behind every contig) and pieces.
__global__ __launch_bounds__(1024) void
k_apply_scan(ApplyArgs a)
{
	__shared__ u64 s_bytes[1024], s_pieces[1024], s_applied[1024];
	const u32 t = threadIdx.x;
	const u32 per = (a.n_contigs + 1023) / 1024;
	const u32 c0 = t * per < a.n_contigs ? t * per : a.n_contigs;
	const u32 c1 = c0 + per < a.n_contigs ? c0 + per : a.n_contigs;
	u64 nb = 0, np = 0, na = 0;
	for (u32 c = c0; c < c1; c++) {
		nb += a.contig[c].out_len + 1;
		np += a.contig[c].n_pieces;
		na += a.contig[c].applied;
	}
	s_bytes[t] = nb;
	s_pieces[t] = np;
	s_applied[t] = na;
	__syncthreads();
	for (u32 d = 1; d < 1024; d <<= 1) {
		u64 vb = 0, vp = 0, va = 0;
		if (t >= d) {
			vb = s_bytes[t - d];
			vp = s_pieces[t - d];
			va = s_applied[t - d];
		}
		__syncthreads();
		s_bytes[t] += vb;
		s_pieces[t] += vp;
		s_applied[t] += va;
		__syncthreads();
	}
	u64 ob = s_bytes[t] - nb, op = s_pieces[t] - np;
	for (u32 c = c0; c < c1; c++) {
		a.out_offs[c] = ob;
		a.out_lens[c] = (u32)a.contig[c].out_len;
		a.piece_base[c] = op;
		ob += a.contig[c].out_len + 1;
		op += a.contig[c].n_pieces;
	}
	if (t == 1023) {
		a.totals[0] = s_bytes[t];
		a.totals[1] = s_pieces[t];
		a.totals[2] = s_applied[t];
		a.piece_base[a.n_contigs] = s_pieces[t];
	}
}

// ----------------------------------------------------------------------------------------------- k_apply_pieces
// Thread per applied event: the pieces of its nodes but the last (which the next applied event's first node replaces,
// or k_apply_tail writes).
__global__ __launch_bounds__(APPLY_TPB) void
k_apply_pieces(ApplyArgs a, u64 total_pieces)
{
	const u32 i = blockIdx.x * APPLY_TPB + threadIdx.x;
	if (i >= a.n_events) {
		return;
	}
	const ApplyPlace pl = a.place[i];
	if ((pl.flags & 3) != 3) {
		return;
	}
	const ApplyEvent ev = a.ev[i];
	if (ev.n_nodes < 2) {
		return;
	}
	const u32 ci = ev.contig;
	const u32 len = a.lens[ci];
	const u64 gbase = a.offs[ci];
	const u64 p_end = a.piece_base[ci + 1];
	u64 o = a.out_offs[ci] + pl.out_off;
	u64 pi = a.piece_base[ci] + pl.piece;
	u64 key = gbase + pl.open_s;
	u32 t = 0;
	(void)walk_event(a.arena, a.arena_items, a.ev_first[i], [&](const Item& it, u32 tag) {
		if (tag != TAG_NODE) {
			return true;
		}
		if (t + 1 >= ev.n_nodes || pi >= p_end || pi >= total_pieces) {
			return false;
		}
		ANode nd = node_of(it);
		if (t == 0 && nd.type == 0 && nd.s == 0) {
			nd.s = pl.open_s;
		}
		u32 err = 0;
		const u32 l = node_len(nd.type, nd.s, nd.e, len, err);
		ApplyPiece p;
		p.out_off = o;
		if (nd.type == 0 && !err) {
			p.src = gbase + nd.s;
			key = gbase + nd.e + 1;
		} else {
			p.src = APPLY_LIT | (key << 8) | (nd.c & 0xFF);
		}
		a.pieces[pi] = p;
		o += l;
		pi++;
		t++;
		return true;
	});
}

// thread per contig: the node that ends its rope, and its separator; the last thread also the table's closing entry
__global__ __launch_bounds__(APPLY_TPB) void
k_apply_tail(ApplyArgs a, u64 total_bytes, u64 total_pieces)
{
	const u32 ci = blockIdx.x * APPLY_TPB + threadIdx.x;
	if (ci >= a.n_contigs) {
		return;
	}
	const ApplyContig c = a.contig[ci];
	const u64 gbase = a.offs[ci];
	const u64 o = a.out_offs[ci];
	const u64 pi = a.piece_base[ci] + c.n_pieces - 2;
	if (pi + 2 <= total_pieces) {
		const int type = (int)(int8_t)(c.open & 0xFF);
		ApplyPiece p;
		p.out_off = o + c.open_off;
		u64 key = gbase + c.open_s;
		if (type == 0 && c.out_len > c.open_off) {
			p.src = gbase + c.open_s;
			key = gbase + c.open_e + 1;
		} else {
			p.src = APPLY_LIT | (key << 8) | ((c.open >> 8) & 0xFF);
		}
		a.pieces[pi] = p;
		ApplyPiece s;
		s.out_off = o + c.out_len;
		s.src = APPLY_LIT | (key << 8) | (u64)'\n';
		a.pieces[pi + 1] = s;
	}
	if (ci == a.n_contigs - 1) {
		ApplyPiece z;
		z.out_off = total_bytes;
		z.src = APPLY_LIT | ((a.n_seq & 0x7FFFFFFFFFFFFFull) << 8);
		a.pieces[total_pieces] = z;
	}
}

// ------------------------------------------------------------------------------------------------- k_apply_copy
// Tiles of APPLY_TILE output bytes, whatever pieces they are made of: an untouched contig of 100 Mbp is 6,400 tiles of one
// piece, a stretch of short pieces a tile that finds its few dozen pieces by binary search in the scanned table (in LDS
// when they fit).  Every thread writes aligned 16-byte chunks; a chunk inside one position node is read with two aligned
// 16-byte loads and shifted, everything else byte by byte.
__device__ __forceinline__ u64
funnel(u64 lo, u64 hi, u32 bits)
{
	return bits ? (lo >> bits) | (hi << (64 - bits)) : lo;
}

__global__ __launch_bounds__(APPLY_TPB) void
k_apply_copy(const ApplyPiece* __restrict__ pieces, u64 n_pieces, const u8* __restrict__ seq, u64 n_seq, u8* __restrict__ out, u64 total)
{
	__shared__ ApplyPiece s_p[APPLY_LDS_PIECES + 1];
	__shared__ u64 s_range[2];
	const u64 t0 = (u64)blockIdx.x * APPLY_TILE;
	const u64 t1 = t0 + APPLY_TILE < total ? t0 + APPLY_TILE : total;
	if (threadIdx.x < 2) {
		// the last piece that begins at or in front of the tile's first (threadIdx 0) / last (1) byte
		const u64 x = threadIdx.x ? t1 - 1 : t0;
		u64 lo = 0, hi = n_pieces; // pieces[n_pieces] closes the table at `total`
		while (lo < hi) {
			const u64 mid = (lo + hi + 1) >> 1;
			if (pieces[mid].out_off <= x) {
				lo = mid;
			} else {
				hi = mid - 1;
			}
		}
		s_range[threadIdx.x] = lo < n_pieces ? lo : n_pieces - 1;
	}
	__syncthreads();
	const u64 p_lo = s_range[0], p_hi = s_range[1];
	const u64 np = p_hi - p_lo + 1;
	const bool in_lds = np <= APPLY_LDS_PIECES;
	if (in_lds) {
		for (u64 q = threadIdx.x; q <= np; q += APPLY_TPB) {
			s_p[q] = pieces[p_lo + q];
		}
	}
	__syncthreads();
	const ApplyPiece* tab = in_lds ? s_p : pieces + p_lo; // tab[0 .. np], tab[np] = the piece behind the tile's last
	for (u32 ch = threadIdx.x; ch < APPLY_TILE / 16; ch += APPLY_TPB) {
		const u64 o = t0 + (u64)ch * 16;
		if (o >= t1) {
			break;
		}
		u64 lo = 0, hi = np - 1;
		while (lo < hi) {
			const u64 mid = (lo + hi + 1) >> 1;
			if (tab[mid].out_off <= o) {
				lo = mid;
			} else {
				hi = mid - 1;
			}
		}
		u64 p = lo;
		ApplyPiece pc = tab[p];
		u64 p_next = tab[p + 1].out_off;
		u64 r0 = 0, r1 = 0;
		const u64 src = pc.src + (o - pc.out_off);
		const u64 a16 = src & ~15ULL;
		if (!(pc.src & APPLY_LIT) && o + 16 <= p_next && a16 + 32 <= n_seq) {
			const uint4 A = *reinterpret_cast<const uint4*>(seq + a16);
			const u64 w0 = (u64)A.x | ((u64)A.y << 32), w1 = (u64)A.z | ((u64)A.w << 32);
			const u32 sh = (u32)(src & 15);
			if (sh == 0) {
				r0 = w0;
				r1 = w1;
			} else {
				const uint4 B = *reinterpret_cast<const uint4*>(seq + a16 + 16);
				const u64 w2 = (u64)B.x | ((u64)B.y << 32), w3 = (u64)B.z | ((u64)B.w << 32);
				if (sh < 8) {
					r0 = funnel(w0, w1, sh * 8);
					r1 = funnel(w1, w2, sh * 8);
				} else {
					r0 = funnel(w1, w2, (sh - 8) * 8);
					r1 = funnel(w2, w3, (sh - 8) * 8);
				}
			}
		} else {
			for (u32 bi = 0; bi < 16; bi++) {
				const u64 oo = o + bi;
				u64 byte = 0;
				if (oo < total) {
					while (oo >= p_next && p + 1 < np) {
						p++;
						pc = tab[p];
						p_next = tab[p + 1].out_off;
					}
					if (pc.src & APPLY_LIT) {
						byte = pc.src & 0xFF;
					} else {
						const u64 g = pc.src + (oo - pc.out_off);
						byte = g < n_seq ? seq[g] : 0;
					}
				}
				if (bi < 8) {
					r0 |= byte << (8 * bi);
				} else {
					r1 |= byte << (8 * (bi - 8));
				}
			}
		}
		uint4 v;
		v.x = (u32)r0;
		v.y = (u32)(r0 >> 32);
		v.z = (u32)r1;
		v.w = (u32)(r1 >> 32);
		*reinterpret_cast<uint4*>(out + o) = v; // (the buffer is a multiple of 16 bytes long; bytes behind `total` are 0)
	}
}

// ------------------------------------------------------------------------------------------------- k_apply_mods
// TAG_MOD items (substitutions, -a soft masks, -m lower-casing) overwrite single bases of the draft -- render_contig's
// copy of it; here the byte of the output that came from that draft position, if the rope kept it.  An applied event's
// MODs count whether its nodes do or not.  The pieces of a contig are ordered by draft position (a rope only moves
// forward), so the piece is found by binary search on the pieces' keys; an event's MODs are applied in its own order by
// one thread, and the runs of two applied events do not overlap.
__global__ __launch_bounds__(APPLY_TPB) void
k_apply_mods(ApplyArgs a, u64 total_bytes)
{
	const u32 i = blockIdx.x * APPLY_TPB + threadIdx.x;
	if (i >= a.n_events) {
		return;
	}
	if (!(a.place[i].flags & 1)) {
		return;
	}
	const u32 ci = a.ev[i].contig;
	const u32 len = a.lens[ci];
	const u64 gbase = a.offs[ci];
	const u64 pb = a.piece_base[ci], pe = a.piece_base[ci + 1];
	(void)walk_event(a.arena, a.arena_items, a.ev_first[i], [&](const Item& it, u32 tag) {
		if (tag != TAG_MOD || it.w[1] >= len) {
			return true;
		}
		const u64 g = gbase + it.w[1];
		u64 lo = pb, hi = pe - 1; // the last piece whose key is <= g
		while (lo < hi) {
			const u64 mid = (lo + hi + 1) >> 1;
			const u64 s = a.pieces[mid].src;
			const u64 key = (s & APPLY_LIT) ? (s & ~APPLY_LIT) >> 8 : s;
			if (key <= g) {
				lo = mid;
			} else {
				hi = mid - 1;
			}
		}
		const ApplyPiece p = a.pieces[lo];
		const u64 plen = a.pieces[lo + 1].out_off - p.out_off;
		if (!(p.src & APPLY_LIT) && g >= p.src && g - p.src < plen && p.out_off + (g - p.src) < total_bytes) {
			a.out[p.out_off + (g - p.src)] = (u8)((it.w[0] >> 8) & 0xFF);
		}
		return true;
	});
}

// ---------------------------------------------------------------------------------------------------- QV counts
__global__ __launch_bounds__(256) void
k_qv_rows(QvRow* rows, const u32* __restrict__ lens_before, const u32* __restrict__ lens_after, u32 n)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) {
		QvRow r;
		r.len_before = lens_before[i];
		r.len_after = lens_after[i];
		r.kmers_before = r.absent_before = r.kmers_after = r.absent_after = 0;
		rows[i] = r;
	}
}

// A, C, G, T in either case: the bases a k-mer of a read set is made of.  (The screening also hashes k-mers that hold one
// of the other IUPAC codes -- with zero seeds, so that they are practically never in a filter; they are no k-mers here.)
__device__ __forceinline__ bool
accepted(u32 c)
{
	const u32 u = (c & 0xDF) - 'A';
	constexpr u32 SET = (1u << 0) | (1u << 2) | (1u << 6) | (1u << 19);
	return u < 26 && ((SET >> u) & 1);
}

// One workgroup per tile of QV_TILE positions of the batch, one bitmap word per thread -- whatever entries the tile holds:
// an entry of 100 Mbp is 6,100 tiles, three thousand contigs of 500 bases are 94.  Phase 1: every thread turns its 64 bytes
// into a word of "A, C, G or T inside an entry" bits, in LDS, the first threads also the ceil((k - 1) / 64) + 1 words of
// look-ahead behind the tile (a run of such bases that crosses the tile's end is followed there, as the reads
// kernels follow their halo).  Phase 2: a position starts a k-mer iff the next k bits are set: the distance to the
// next clear bit, carried backwards through the word from the words behind it.  Those bits and the absent bitmap's are
// counted per entry; what falls into the entry the tile begins in is reduced over the workgroup and added with one
// 64-bit atomic per count, every other entry begins in this tile and takes the atomics of its own words only.
__global__ __launch_bounds__(QV_TPB) void
k_qv_count(const u8* __restrict__ seq, u64 n, const u64* __restrict__ offs, const u32* __restrict__ lens, u32 n_entries,
           const u64* __restrict__ bitmap, u32 k, QvRow* rows, int which)
{
	__shared__ u64 s_good[QV_TPB + QV_MAX_K / 64 + 2];
	__shared__ unsigned long long s_sum[2];
	const u64 t0 = (u64)blockIdx.x * QV_TILE;
	const u32 halo_words = (k - 1 + 63) / 64 + 1;
	const u32 n_good = QV_TPB + halo_words;
	if (threadIdx.x < 2) {
		s_sum[threadIdx.x] = 0;
	}
	for (u32 w = threadIdx.x; w < n_good; w += QV_TPB) {
		const u64 p0 = t0 + (u64)w * 64;
		u64 acc = 0;
		if (p0 < n) {
			if (p0 + 64 <= n) {
				const uint4* src = reinterpret_cast<const uint4*>(seq + p0);
				for (u32 q = 0; q < 4; q++) {
					const uint4 v = src[q];
					const u32 d[4] = { v.x, v.y, v.z, v.w };
					for (u32 j = 0; j < 4; j++) {
						for (u32 bb = 0; bb < 4; bb++) {
							acc |= (u64)accepted((d[j] >> (8 * bb)) & 0xFF) << (q * 16 + j * 4 + bb);
						}
					}
				}
			} else {
				for (u32 bb = 0; p0 + bb < n; bb++) {
					acc |= (u64)accepted(seq[p0 + bb]) << bb;
				}
			}
			// inside an entry
			u64 inside = 0;
			for (u32 e = entry_behind(offs, lens, n_entries, p0); e < n_entries && offs[e] < p0 + 64; e++) {
				const u64 a0 = offs[e] > p0 ? offs[e] - p0 : 0;
				const u64 a1 = offs[e] + lens[e] - p0;
				inside |= bit_range((u32)a0, (u32)(a1 < 64 ? a1 : 64));
			}
			acc &= inside;
		}
		s_good[w] = acc;
	}
	__syncthreads();
	const u32 w = threadIdx.x;
	const u64 p0 = t0 + (u64)w * 64;
	const u32 e_tile = entry_behind(offs, lens, n_entries, t0); // the entry the tile begins in (or the first behind its start)
	unsigned long long my_k = 0, my_a = 0;
	if (p0 < n) {
		// distance from position p0 + 64 to the next clear bit, up to k
		u32 d = 0;
		for (u32 q = w + 1; q < n_good && d < k; q++) {
			const u64 g = s_good[q];
			if (g == ~0ULL) {
				d += 64;
			} else {
				d += (u32)__ffsll((unsigned long long)~g) - 1;
				break;
			}
		}
		const u64 g = s_good[w];
		u64 starts = 0;
		for (int bb = 63; bb >= 0; bb--) {
			d = ((g >> bb) & 1) ? d + 1 : 0;
			starts |= (u64)(d >= k) << bb;
		}
		const u64 absent = bitmap[p0 / 64];
		for (u32 e = entry_behind(offs, lens, n_entries, p0); e < n_entries && offs[e] < p0 + 64; e++) {
			const u64 a0 = offs[e] > p0 ? offs[e] - p0 : 0;
			const u64 a1 = offs[e] + lens[e] - p0;                                    // end of the entry
			const u64 s1 = lens[e] >= k ? offs[e] + lens[e] - k + 1 : offs[e];         // end of its k-mer starts
			const u64 m_all = bit_range((u32)a0, (u32)(a1 < 64 ? a1 : 64));
			const u64 m_st = s1 > p0 ? bit_range((u32)a0, (u32)(s1 - p0 < 64 ? s1 - p0 : 64)) : 0;
			const unsigned long long nk = (unsigned long long)__popcll(starts & m_all);
			const unsigned long long na = (unsigned long long)__popcll(absent & m_st);
			if (e == e_tile) {
				my_k += nk;
				my_a += na;
			} else {
				unsigned long long* r = reinterpret_cast<unsigned long long*>(rows + e);
				if (nk) {
					atomicAdd(r + (which ? 4 : 2), nk);
				}
				if (na) {
					atomicAdd(r + (which ? 5 : 3), na);
				}
			}
		}
	}
	// the tile's own entry: wavefront reduction, one LDS atomic per wavefront, one global atomic per count
	for (int o = 32; o > 0; o >>= 1) {
		my_k += __shfl_down(my_k, o);
		my_a += __shfl_down(my_a, o);
	}
	if ((threadIdx.x & 63) == 0) {
		atomicAdd(&s_sum[0], my_k);
		atomicAdd(&s_sum[1], my_a);
	}
	__syncthreads();
	if (threadIdx.x == 0 && e_tile < n_entries) {
		unsigned long long* r = reinterpret_cast<unsigned long long*>(rows + e_tile);
		if (s_sum[0]) {
			atomicAdd(r + (which ? 4 : 2), s_sum[0]);
		}
		if (s_sum[1]) {
			atomicAdd(r + (which ? 5 : 3), s_sum[1]);
		}
	}
}

} // namespace

void
launch_apply_plan(hipStream_t stream, const ApplyArgs& a)
{
	if (a.n_events) {
		hipLaunchKernelGGL(k_apply_summary, dim3((a.n_events + APPLY_TPB - 1) / APPLY_TPB), dim3(APPLY_TPB), 0, stream, a);
	}
	const u32 per = APPLY_TPB / 64;
	hipLaunchKernelGGL(k_apply_chain, dim3((a.n_contigs + per - 1) / per), dim3(APPLY_TPB), 0, stream, a);
	hipLaunchKernelGGL(k_apply_scan, dim3(1), dim3(1024), 0, stream, a);
}

void
launch_apply_write(hipStream_t stream, const ApplyArgs& a, u64 total_bytes, u64 total_pieces)
{
	if (a.n_events) {
		hipLaunchKernelGGL(k_apply_pieces, dim3((a.n_events + APPLY_TPB - 1) / APPLY_TPB), dim3(APPLY_TPB), 0, stream, a, total_pieces);
	}
	hipLaunchKernelGGL(k_apply_tail, dim3((a.n_contigs + APPLY_TPB - 1) / APPLY_TPB), dim3(APPLY_TPB), 0, stream, a, total_bytes, total_pieces);
	const u64 tiles = (total_bytes + APPLY_TILE - 1) / APPLY_TILE;
	if (tiles) {
		hipLaunchKernelGGL(k_apply_copy, dim3((unsigned)tiles), dim3(APPLY_TPB), 0, stream, a.pieces, total_pieces, a.seq, a.n_seq, a.out, total_bytes);
	}
	if (a.n_events) {
		hipLaunchKernelGGL(k_apply_mods, dim3((a.n_events + APPLY_TPB - 1) / APPLY_TPB), dim3(APPLY_TPB), 0, stream, a, total_bytes);
	}
}

void
launch_qv_rows(hipStream_t stream, QvRow* rows, const u32* lens_before, const u32* lens_after, u32 n)
{
	if (n) {
		hipLaunchKernelGGL(k_qv_rows, dim3((n + 255) / 256), dim3(256), 0, stream, rows, lens_before, lens_after, n);
	}
}

void
launch_qv_count(hipStream_t stream, const u8* seq, u64 n, const u64* offs, const u32* lens, u32 n_entries, const u64* bitmap, u32 k, QvRow* rows,
                int which)
{
	const u64 tiles = (n + QV_TILE - 1) / QV_TILE;
	if (tiles && n_entries) {
		hipLaunchKernelGGL(k_qv_count, dim3((unsigned)tiles), dim3(QV_TPB), 0, stream, seq, n, offs, lens, n_entries, bitmap, k, rows, which);
	}
}

} // namespace nte
