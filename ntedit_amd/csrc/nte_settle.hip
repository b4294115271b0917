// nte_settle.hip -- k_settle: the plain substitution events of a round, settled ahead of the thread-per-event launch.
//
// The lanes of k_machine<false, .> part at the first data-dependent branch of the general machine; after that a
// wavefront has one lane's probe group in flight.  Here every lane asks the same fixed question, settle_event()
// (nte_settle.h), about its event: the candidates' own k-mers together, then the k rolls of a present candidate in
// groups of NTE_SETTLE_GROUP, level by level.  An event it accepts gets its arena chunk, first_chunk, cover end and
// flags exactly as the machine would have left them; the others are appended to the rest list, which the unchanged
// thread-per-event launch runs.
#include "nte_settle.h"
#include "nte_machine_launch.h"

#include <hip/hip_runtime.h>

namespace nte {

#ifndef NTE_SETTLE_GROUP
#define NTE_SETTLE_GROUP 8 // k-mers a lane probes together
#endif
#ifndef NTE_SETTLE_MIN_BLOCKS
#define NTE_SETTLE_MIN_BLOCKS 4
#endif

#if defined(NTE_PROFILE)
static __device__ unsigned long long g_settle_gathers;
#endif

__global__ __launch_bounds__(MACHINE_TPB, NTE_SETTLE_MIN_BLOCKS) void
k_settle(MachineArgs a, u32* rest, u32* n_rest)
{
	__shared__ __attribute__((aligned(16))) u64 s_tab[TAB_WORDS];
	extern __shared__ __attribute__((aligned(16))) u8 s_win[]; // 2k codes per lane, interleaved (byte i of lane t at i * 256 + t)
	if (threadIdx.x < TAB_WORDS) {
		s_tab[threadIdx.x] = a.tabs[threadIdx.x];
	}
	__syncthreads();
	EventEnv env;
	env.bitmap = a.bitmap;
	env.runmap = a.runmap;
	env.tab = s_tab;
	env.p = &a.p;
	env.bloom = a.bloom;
	env.rep = a.rep;
	env.nodes = nullptr;
	env.ov_pos = nullptr;
	env.ov_chr = nullptr;
	env.win = s_win + threadIdx.x;
	env.win_stride = MACHINE_TPB;
	env.prev = nullptr;
	env.lps = nullptr;
	env.arena = a.arena;
	env.arena_next = a.arena_next;
	env.arena_chunks = a.arena_chunks;
	env.defer_sweeps = false;
	env.wave_size = 1;
	env.batch_end = a.seq + a.n_bytes;
	const u32 lane = threadIdx.x & 63u;
	const u64 below = (1ULL << lane) - 1;
	for (u64 base = (u64)blockIdx.x * MACHINE_TPB; base < a.n_events; base += (u64)gridDim.x * MACHINE_TPB) {
		const u64 it = base + threadIdx.x;
		const bool have = it < a.n_events;
		u32 ev = 0;
		bool accepted = false;
		SettleOut out;
		u64 cover_g = 0;
		if (have) {
			ev = a.ev_list ? a.ev_list[it] : (u32)it;
			const u64 g = a.events[ev];
			// contig of g: last offset <= g
			u32 lo = 0, hi = a.n_contigs;
			while (hi - lo > 1) {
				const u32 mid = lo + ((hi - lo) >> 1);
				if (a.offsets[mid] <= g) {
					lo = mid;
				} else {
					hi = mid;
				}
			}
			env.contig = lo;
			env.gbase = a.offsets[lo];
			env.seq = a.seq + env.gbase;
			env.len = a.lens[lo];
			const u32 start = (u32)(g - env.gbase);
			SettleMachine m(env);
			accepted = settle_event_on<NTE_SETTLE_GROUP>(m, start, out);
			cover_g = env.gbase + out.cover_end;
#if defined(NTE_PROFILE) && defined(__HIP_DEVICE_COMPILE__)
			if (m.prof_gathers) {
				atomicAdd(&g_settle_gathers, m.prof_gathers);
			}
#endif
		}
		// one bump of the arena cursor and one of the rest list per wavefront
		const u64 acc = __ballot(accepted), dec = __ballot(have && !accepted);
		u32 chunk0 = 0, rest0 = 0;
		if (lane == 0) {
			if (acc) {
				chunk0 = atomicAdd(a.arena_next, (u32)__popcll(acc));
			}
			if (dec) {
				rest0 = atomicAdd(n_rest, (u32)__popcll(dec));
			}
		}
		chunk0 = (u32)__shfl((int)chunk0, 0, 64);
		rest0 = (u32)__shfl((int)rest0, 0, 64);
		if (accepted) {
			const u32 chunk = chunk0 + (u32)__popcll(acc & below);
			u32 fc = NONE32;
			if (chunk >= a.arena_chunks || chunk < chunk0) {
				atomicOr(a.status, (u32)EV_ARENA_FULL); // (the batch is run again with more room)
			} else {
				uint4* dst = reinterpret_cast<uint4*>(a.arena + (u64)chunk * CHUNK_ITEMS);
				NTE_UNROLL
				for (int i = 0; i < 4; i++) {
					dst[i] = make_uint4(out.item[i].w[0], out.item[i].w[1], out.item[i].w[2], out.item[i].w[3]);
				}
				fc = chunk;
			}
			a.first_chunk[ev] = fc;
			if (a.ev_cover) {
				a.ev_cover[ev] = cover_g;
				a.ev_flags[ev] = (u8)(a.ev_flags[ev] | 0x80u); // ran to its end
			}
		} else if (have) {
			rest[rest0 + (u32)__popcll(dec & below)] = ev;
		}
	}
}

// dyn LDS: 2k bytes per thread
void
launch_k_settle(unsigned blocks, hipStream_t stream, const MachineArgs& a, u32* rest, u32* n_rest)
{
	hipLaunchKernelGGL(k_settle, dim3(blocks), dim3(MACHINE_TPB), (size_t)2 * a.p.k * MACHINE_TPB, stream, a, rest, n_rest);
}

// filter gathers counted by a -DNTE_PROFILE build (0 otherwise); reading resets the counter
unsigned long long
settle_gathers()
{
	unsigned long long v = 0;
#if defined(NTE_PROFILE)
	unsigned long long zero = 0;
	(void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_settle_gathers), sizeof v);
	(void)hipMemcpyToSymbol(HIP_SYMBOL(g_settle_gathers), &zero, sizeof zero);
#endif
	return v;
}

} // namespace nte
