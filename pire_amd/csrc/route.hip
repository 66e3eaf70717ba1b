// From end states to one hit list PER REGEXP on the device (pire_hip_route): the fork behind a glued scanner.
//
// The compaction of its sibling unit answers "which strings matched anything (or anything in `want`)" as ONE ascending
// list.  A caller of a scanner of R glued regexps asks R such questions at once: for every regexp r, the ascending list
// of the strings whose end state has r in AcceptedRegexps (multi.h:149-158).  This unit answers all of them in one pass
// over the state indices, into a fixed-pitch layout the gather entry points can chain on without a read-back:
//
//   out_hits[R][hit_cap]   row r: the indices i with member(i, r), ascending; only min(count[r], hit_cap) entries written
//   out_hit_counts[R]      the full counts
//
//   count     one lane per string, tiles of 1 024 strings: state index -> mask record.  Per mask word the wave forms the
//             OR of its 64 lanes (wave-uniform, in scalar registers) and walks ONLY the regexps that occur in the wave:
//             one ballot + popcount each.  The per-wave counts meet in LDS, 64 regexps (one mask word) a round, so no
//             number of regexps outgrows the LDS; tileCounts[r][tile] is written for every r, zeros included.
//   scan      R independent exclusive scans of `tiles` entries, a block per regexp (grid-stride), 1 024 entries a step
//             with a carry; the total of row r is out_hit_counts[r] (select.hip's kernel, LaunchTileScan with R rows).
//   scatter   re-reads the state indices and the mask records (no ballot scratch): rank = scanned tile offset + the same
//             regexp's popcounts of the waves in front (an LDS phase) + mbcnt of the wave's own ballot.
//
// Three launches on the caller's stream; no block ever waits for another block, no atomics: the order inside a row is the
// order of the strings, whatever the timing.  The image is the select pass's (internal.h SelectHost: reference numbering,
// no re-ranking touches it).  Plain HIP with compiler-placed waits.  The lines form adds the byte ranges of all rows in one
// launch over (r, k): split.hip's SplitSpansKernel, LaunchHitSpans.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"

namespace pirehip {

namespace {

constexpr uint32_t kRouteThreads = 1024;           // one tile = 1 024 strings = 16 waves
constexpr uint32_t kRouteWaves = kRouteThreads / 64;
constexpr uint32_t kRouteMaxBlocks = 8192;

struct RouteParams {
	const uint64_t* masks;   // [states * words], reference numbering
	uint32_t states, words, regexps;
	const uint32_t* stateIdx;
	uint64_t n;
	uint32_t* tileCounts;    // [regexps][tiles]: members per tile; after the scan: members in front of the tile
	uint32_t tiles;
	uint64_t* outHits;       // [regexps][hitCap]
	uint64_t hitCap;
};

// The OR of m over the wave's 64 lanes, in scalar registers: the loops over its set bits are scalar loops
__device__ __forceinline__ uint64_t WaveOr(uint64_t m)
{
	uint32_t lo = uint32_t(m), hi = uint32_t(m >> 32);
	for (uint32_t d = 1; d < 64; d <<= 1) {
		lo |= uint32_t(__shfl_xor(int(lo), int(d), 64));
		hi |= uint32_t(__shfl_xor(int(hi), int(d), 64));
	}
	lo = uint32_t(__builtin_amdgcn_readfirstlane(int(lo)));
	hi = uint32_t(__builtin_amdgcn_readfirstlane(int(hi)));
	return (uint64_t(hi) << 32) | lo;
}

// Lane b's value: how many lanes of the wave have bit b of m, for the bits of `present` (the wave's OR); 0 elsewhere
__device__ __forceinline__ uint32_t WaveBitCounts(uint64_t m, uint64_t present, uint32_t lane)
{
	uint32_t mine = 0;
	while (present) {
		const uint32_t b = uint32_t(__builtin_ctzll(present));
		present &= present - 1;
		const uint32_t c = uint32_t(__popcll(__ballot((m >> b) & 1)));
		mine = lane == b ? c : mine;
	}
	return mine;
}

// A string behind the batch's end, and a state index beyond the table (undefined behaviour of the ON_DEVICE form; the
// host-pointer form refuses it), read nothing: state ~0 / an empty mask, a member of no row.
__device__ __forceinline__ uint32_t RouteState(const RouteParams& p, uint64_t i)
{
	return i < p.n ? p.stateIdx[i] : ~0u;
}
__device__ __forceinline__ uint64_t RouteMask(const RouteParams& p, uint32_t s, uint32_t w)
{
	// (the image has no bit at or above `regexps`; the rows that are written must not depend on that)
	const uint32_t left = p.regexps - w * 64;
	const uint64_t valid = left >= 64 ? ~0ull : (1ull << left) - 1;
	return s < p.states ? p.masks[size_t(s) * p.words + w] & valid : 0;
}

__global__ __launch_bounds__(kRouteThreads) void RouteCountKernel(RouteParams p)
{
	__shared__ uint32_t waveCount[kRouteWaves][64];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
		const uint32_t s = RouteState(p, uint64_t(tile) * kRouteThreads + threadIdx.x);
		for (uint32_t w = 0; w < p.words; ++w) {
			const uint64_t m = RouteMask(p, s, w);
			waveCount[wave][lane] = WaveBitCounts(m, WaveOr(m), lane);
			__syncthreads();
			const uint32_t r = w * 64 + threadIdx.x;
			if (threadIdx.x < 64 && r < p.regexps) {
				uint32_t sum = 0;
				for (uint32_t k = 0; k < kRouteWaves; ++k)
					sum += waveCount[k][threadIdx.x];
				p.tileCounts[size_t(r) * p.tiles + tile] = sum;
			}
			__syncthreads();
		}
	}
}

__global__ __launch_bounds__(kRouteThreads) void RouteScatterKernel(RouteParams p)
{
	__shared__ uint32_t waveBase[kRouteWaves][64];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
		const uint64_t i = uint64_t(tile) * kRouteThreads + threadIdx.x;
		const uint32_t s = RouteState(p, i);
		for (uint32_t w = 0; w < p.words; ++w) {
			const uint64_t m = RouteMask(p, s, w);
			const uint64_t present = WaveOr(m);
			waveBase[wave][lane] = WaveBitCounts(m, present, lane);
			__syncthreads();
			// the first wave, a lane per regexp of this word: from the waves' counts to the rank of every wave's first member
			const uint32_t r = w * 64 + threadIdx.x;
			if (threadIdx.x < 64 && r < p.regexps) {
				uint32_t running = p.tileCounts[size_t(r) * p.tiles + tile];
				for (uint32_t k = 0; k < kRouteWaves; ++k) {
					const uint32_t c = waveBase[k][threadIdx.x];
					waveBase[k][threadIdx.x] = running;
					running += c;
				}
			}
			__syncthreads();
			for (uint64_t bits = present; bits; bits &= bits - 1) {
				const uint32_t b = uint32_t(__builtin_ctzll(bits));
				const bool member = (m >> b) & 1;
				const uint64_t ballot = __ballot(member);
				const uint64_t rank = uint64_t(waveBase[wave][b]) +
				                      __builtin_amdgcn_mbcnt_hi(uint32_t(ballot >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(ballot), 0));
				if (member && rank < p.hitCap)
					p.outHits[uint64_t(w * 64 + b) * p.hitCap + rank] = i;
			}
			__syncthreads();
		}
	}
}

}  // namespace

int LaunchRoute(const SelectDevice& image, uint32_t states, uint32_t words, uint32_t regexps, const uint32_t* stateIdx, uint64_t n,
                uint64_t* outHits, uint64_t hitCap, uint64_t* outHitCounts, hipStream_t stream)
{
	if (regexps == 0)
		return PIRE_HIP_OK;
	if (n == 0) {
		const hipError_t e = hipMemsetAsync(outHitCounts, 0, size_t(regexps) * 8, stream);
		return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemsetAsync(hit counts)");
	}
	if (n >= (1ull << 32)) {
		SetError("pire_hip_route: 2^32 strings or more in one call");   // tile offsets are 32 bits
		return PIRE_HIP_EUNSUPPORTED;
	}
	RouteParams p;
	p.masks = image.masks;
	p.states = states;
	p.words = words;
	p.regexps = regexps;
	p.stateIdx = stateIdx;
	p.n = n;
	p.tiles = uint32_t((n + kRouteThreads - 1) / kRouteThreads);
	p.outHits = outHits;
	p.hitCap = outHits ? hitCap : 0;
	// scratch: regexps * n / 256 bytes of tile counts and nothing else, stream-ordered (the call only enqueues)
	StreamScratch scratch(stream);
	if (int rc = scratch.Alloc(size_t(regexps) * p.tiles * 4, "hipMallocAsync(route scratch)"))
		return rc;
	p.tileCounts = scratch.as<uint32_t>();
	const dim3 grid(std::min(p.tiles, kRouteMaxBlocks));
	hipLaunchKernelGGL(RouteCountKernel, grid, dim3(kRouteThreads), 0, stream, p);
	LaunchTileScan(p.tileCounts, regexps, p.tiles, outHitCounts, stream);
	if (p.hitCap)
		hipLaunchKernelGGL(RouteScatterKernel, grid, dim3(kRouteThreads), 0, stream, p);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "route launch");
}

}  // namespace pirehip
