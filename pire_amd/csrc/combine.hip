// Boolean queries over hit lists on the device (pire_hip_combine): grep a | grep -v b, two columns, two kinds of scanner.
//
// Every hit pass answers "which lines matched" with an ascending list of line numbers.  This unit puts up to six of them
// together: line i carries the member mask m(i) -- bit j: i is in list j --, and a truth table of 2^k bits says which masks
// are selected.  Bit 0, "in no list", is legal: one list under truth = 1 is its complement.  It takes no table and no text:
// it reads line numbers, whoever wrote them (include/pire_hip.h has the formula).
//
//   classify  one tile = 1 024 LINES, whatever the lists are: a list with 10^6 entries around a tile costs what any other
//             costs.  2 * k waves at once find the slices of the k lists that lie inside the tile, 64 probes a step, every
//             probe clamped into the list.  A slice has at most 1 024 entries; list after list, with a barrier between
//             them, each entry sets bit j of its line's byte of LDS (entries of one list are distinct lines: distinct
//             lanes, distinct bytes, no atomic).  A lane then reads its byte, looks it up in the truth table, and the
//             selected bits of a wave are one ballot word; one count per tile.  Where the caller asks for the masks the
//             byte goes to scratch for the scatter.
//   scan      exclusive scan of the tile counts, one block; the total is the count (select.hip's kernel, LaunchTileScan).
//   scatter   rank of a selected line = tile offset + the popcounts of the waves in front + mbcnt of its own wave's ballot
//             word; the lane writes its index and its member byte.
//
// Scratch, stream-ordered: n / 8 + n / 256 bytes of ballot words and tile counts, and n bytes of member masks where
// out_hit_members is asked for.
//
// The scatter kernel and the launcher are tile_pass.h's, the wave-wide search and the load of a list entry compact.h's
// (WaveBound, LoadU64), the staging of the count and the lists internal.h's HitStage; this unit keeps its classify kernel
// -- it ends in compact.h's TileBallot -- and what a selected lane writes (CombinePass).  Launches on the caller's stream:
// no block waits for another block, no atomics (the same input gives the same bytes).  Plain HIP with compiler-placed waits.  Lists may have any alignment.
// A list that is not ascending or names lines >= n gives an unspecified selection and nothing worse: every index into a
// list is clamped into [0, k_j), every index into the tile's bytes is checked against the tile.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "tile_pass.h"

namespace pirehip {

namespace {

constexpr uint32_t kCmbLists = PIRE_HIP_COMBINE_MAX_LISTS;
static_assert(2 * kCmbLists <= kBlockWaves, "one wave per bound of every list");

struct CombinePass {
	const uint64_t* lists[kCmbLists];    // any alignment
	const uint64_t* counts[kCmbLists];   // nullable: k_j = caps[j]
	uint64_t caps[kCmbLists];
	uint32_t kLists;
	uint64_t n;
	uint64_t truth;
	uint64_t* outHits;       // nullable
	uint8_t* outMembers;     // nullable
	uint8_t* members;        // [tiles * 1024] member masks, or null

	__device__ __forceinline__ void Write(uint64_t rank, uint64_t i) const
	{
		outHits[rank] = i;
		if (outMembers)
			outMembers[rank] = members[i];
	}
};

__global__ __launch_bounds__(kBlockThreads) void CombineClassifyKernel(CombinePass p, TileScratch t)
{
	__shared__ uint32_t waveCount[kBlockWaves];
	__shared__ uint64_t slice[2 * kCmbLists];
	__shared__ uint8_t mark[kBlockThreads];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint32_t tile = blockIdx.x; tile < t.tiles; tile += gridDim.x) {
		const uint64_t t0 = uint64_t(tile) * kBlockThreads, t1 = std::min(t0 + kBlockThreads, p.n);
		const uint64_t i = t0 + threadIdx.x;
		// the slices of the lists inside the tile: wave 2j finds where list j's begins, wave 2j + 1 where it ends
#pragma unroll
		for (uint32_t j = 0; j < kCmbLists; ++j)
			if (j < p.kLists && (wave >> 1) == j) {
				const uint64_t k = std::min(p.counts[j] ? *p.counts[j] : p.caps[j], p.caps[j]);
				const uint64_t at = WaveBound<false>(p.lists[j], k, wave & 1 ? t1 : t0);
				if (lane == 0)
					slice[wave] = at;
			}
		mark[threadIdx.x] = 0;
		__syncthreads();
		// list after list: entries of one list are distinct lines, so distinct lanes write distinct bytes
#pragma unroll
		for (uint32_t j = 0; j < kCmbLists; ++j)
			if (j < p.kLists) {
				const uint64_t lo = slice[2 * j], hi = std::max(slice[2 * j + 1], lo);
				if (threadIdx.x < hi - lo) {
					const uint64_t h = LoadU64(p.lists[j], lo + threadIdx.x);
					if (h >= t0 && h < t1)
						mark[h - t0] |= uint8_t(1u << j);
				}
				__syncthreads();
			}
		const uint32_t m = mark[threadIdx.x];
		const bool sel = i < p.n && ((p.truth >> m) & 1);
		if (p.members)
			p.members[size_t(tile) * kBlockThreads + threadIdx.x] = uint8_t(m);
		TileBallot(sel, tile, t.ballots, t.tileCounts, waveCount);   // (two barriers: slice and mark are free again)
	}
}

}  // namespace

int LaunchCombine(const CombineLists& in, uint64_t n, uint64_t truth, uint64_t* outHits, uint8_t* outMembers, uint64_t hitCap,
                  uint64_t* outHitCount, hipStream_t stream)
{
	TilePass t(stream);
	StreamScratch members(stream);
	const int rc = t.Front("pire_hip_combine", "hipMallocAsync(combine scratch)", n, outHitCount);
	if (rc || !t.s.tiles)
		return rc;
	CombinePass p;
	const uint64_t cap = outHits ? hitCap : 0;
	p.outHits = outHits;
	p.outMembers = outHits ? outMembers : nullptr;
	p.members = nullptr;
	if (p.outMembers && cap) {   // n bytes of member masks, rounded up to whole tiles
		if (int rc2 = members.Alloc(size_t(t.s.tiles) * kBlockThreads, "hipMallocAsync(combine members)"))
			return rc2;
		p.members = members.as<uint8_t>();
	}
	for (uint32_t j = 0; j < kCmbLists; ++j) {
		const bool have = j < in.k;
		p.lists[j] = have ? in.lists[j] : nullptr;
		p.counts[j] = have ? in.counts[j] : nullptr;
		p.caps[j] = have ? in.caps[j] : 0;
	}
	p.kLists = in.k;
	p.n = n;
	p.truth = truth;
	hipLaunchKernelGGL(CombineClassifyKernel, t.Grid(), dim3(kBlockThreads), 0, stream, p, t.s);
	return t.Tail(p, cap, outHitCount, "combine launch");
}

int CombineOutputsInvalid(const char* who, uint64_t n, const CombineOut& o, bool ownList)
{
	const char* what = !o.outHitCount                         ? "null out_hit_count"
	                   : o.hitCap && !o.outHits && !ownList   ? "hit_cap > 0 with null out_hits"
	                   : o.outMembers && !o.outHits           ? "out_hit_members without out_hits"
	                   : n >= (1ull << 32)                    ? "2^32 lines or more in one call"
	                                                          : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

namespace {

int Refuse(const char* who, const std::string& what)
{
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

}  // namespace

}  // namespace pirehip

using namespace pirehip;

extern "C" int pire_hip_combine(const uint64_t* const* lists, const uint64_t* const* list_counts, const uint64_t* list_caps, uint32_t k_lists,
                                uint64_t n, uint64_t truth, uint32_t flags, uint64_t* out_hits, uint8_t* out_hit_members, uint64_t hit_cap,
                                uint64_t* out_hit_count, void* streamPtr)
try {
	const char* who = "pire_hip_combine";
	if (k_lists == 0 || k_lists > PIRE_HIP_COMBINE_MAX_LISTS)
		return Refuse(who, k_lists ? "more than 6 lists" : "k_lists == 0");
	if (!lists || !list_caps)
		return Refuse(who, lists ? "null list_caps" : "null lists");
	for (uint32_t j = 0; j < k_lists; ++j) {
		if (list_caps[j] && !lists[j])
			return Refuse(who, "list_caps[" + std::to_string(j) + "] > 0 with null lists[" + std::to_string(j) + "]");
		if (list_caps[j] >= (1ull << 32))
			return Refuse(who, "2^32 entries or more in list " + std::to_string(j));
	}
	const CombineOut o = {out_hits, out_hit_members, hit_cap, out_hit_count};
	if (int rc = CombineOutputsInvalid(who, n, o))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	CombineLists in = {};
	in.k = k_lists;
	if (flags & PIRE_HIP_RUN_ON_DEVICE) {
		for (uint32_t j = 0; j < k_lists; ++j) {
			in.lists[j] = lists[j];
			in.counts[j] = list_counts ? list_counts[j] : nullptr;
			in.caps[j] = list_caps[j];
		}
		return LaunchCombine(in, n, truth, out_hits, out_hit_members, hit_cap, out_hit_count, stream);
	}
	// host pointers: the lists are looked at, staged in, the kernels, staged out -- the lists only as far as they were written
	uint64_t k[PIRE_HIP_COMBINE_MAX_LISTS] = {};
	for (uint32_t j = 0; j < k_lists; ++j) {
		k[j] = std::min(list_counts && list_counts[j] ? *list_counts[j] : list_caps[j], list_caps[j]);
		uint64_t last = 0;
		for (uint64_t e = 0; e < k[j]; ++e) {
			uint64_t h;   // (a list may have any alignment)
			memcpy(&h, reinterpret_cast<const uint8_t*>(lists[j]) + e * 8, 8);
			if (h >= n)
				return Refuse(who, "list " + std::to_string(j) + " names a line out of range");
			if (e && h <= last)
				return Refuse(who, "list " + std::to_string(j) + " must be strictly ascending");
			last = h;
		}
	}
	if (n == 0) {
		*out_hit_count = 0;
		return PIRE_HIP_OK;
	}
	BatchIO io(stream, false);
	HitStage list(false, out_hit_count, "hipMemcpy(combined hits)");   // n lines: no list is staged longer
	uint64_t* dHits = nullptr;
	uint8_t* dMembers = nullptr;
	int rc;
	for (uint32_t j = 0; j < k_lists; ++j) {
		const uint8_t* d = nullptr;
		if ((rc = io.In(reinterpret_cast<const uint8_t*>(lists[j]), size_t(k[j]) * 8, &d)))
			return rc;
		in.lists[j] = reinterpret_cast<const uint64_t*>(d);
		in.counts[j] = nullptr;
		in.caps[j] = k[j];
	}
	if ((rc = list.Count(io, hit_cap, n)) || (rc = list.List(io, out_hits, 1, &dHits)) || (rc = list.List(io, out_hit_members, 1, &dMembers)) ||
	    (rc = io.Ready()))
		return rc;
	if ((rc = LaunchCombine(in, n, truth, dHits, dMembers, dHits ? list.cap : 0, list.dCount, stream)))
		return rc;
	if ((rc = io.Finish()))
		return rc;
	return list.Back();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}
