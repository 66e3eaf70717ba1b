// From a hit list to the hits and their neighbours on the device (pire_hip_context): grep -A / -B / -C.
//
// Every hit pass answers "which lines matched".  Someone reading a log wants the lines AROUND a match as well: the stack trace
// under an ERROR line, the request above a failed response.  This unit turns an ascending hit list into the ascending list of
// the lines that lie within `after` lines behind or `before` lines in front of a hit, with two bits a line: whether it is a
// hit itself, and whether it begins a run of selected lines (where grep prints its "--").  It takes no table and no text: it
// reads line numbers, whoever wrote them (include/pire_hip.h has the formula).
//
//   classify  one tile = 1 024 LINES, whatever the hits are: a hit with after = 10^6 costs what any other costs.  Two waves
//             find the slice of the hit list that lies inside the tile, 64 probes a step; its at most 1 024 entries set one
//             byte of LDS each (distinct lanes, distinct bytes: no atomic), the bytes become the tile's 16 hit words.  A lane
//             finds the nearest hit at or before its line and the nearest at or after it in those words; where the tile has
//             none on a side, it is the one entry just outside the slice.  selected = i - pred <= after || succ - i <= before
//             (subtractions only: every value of before and after is legal); a run begins where the line in front is not
//             selected -- for the first line of a tile that line's own two neighbours are the same two entries outside the slice.
//             The selected, hit and run bits of a wave are one ballot word each, kept in scratch; two counts per tile.
//   scan      exclusive scan of the tile counts, one block; the total is the line count (select.hip's kernel,
//             LaunchTileScan).  A second launch of it sums the runs where the caller asks for their number.
//   scatter   rank of a selected line = tile offset + the popcounts of the waves in front + mbcnt of its own wave's ballot
//             word; the lane writes its index and its flag byte.
//
// The scatter kernel and the launcher are tile_pass.h's, the wave-wide search and the load of a list entry compact.h's
// (WaveBound, LoadU64), the staging of the count and the lists internal.h's HitStage; this unit keeps its classify kernel --
// it ends in compact.h's TileBallot -- and what a selected lane writes (ContextPass).  Launches on the caller's stream: no
// block waits for another block, no atomics (the same input gives the same bits).  Plain HIP with compiler-placed waits:
// nothing here keeps data on its way in registers.  `hits` may have any alignment: an entry is read through a packed type.  A list that is not ascending or names lines >= n gives an unspecified selection and nothing worse:
// every index into `hits` is clamped into [0, k), every index into the tile's bytes is checked against the tile.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "tile_pass.h"

namespace pirehip {

namespace {

struct ContextPass {
	const uint64_t* hits;       // [k], any alignment
	const uint64_t* hitCount;   // nullable: k = hitCap
	uint64_t hitCap;
	uint64_t n;
	uint64_t before, after;
	uint64_t* outLines;         // nullable
	uint8_t* outFlags;          // nullable
	uint64_t* marks;            // [tiles * 16][2] hit bits and run bits of the wave
	uint32_t* groupCounts;      // [tiles] runs that begin in the tile

	__device__ __forceinline__ void Write(uint64_t rank, uint64_t i) const
	{
		outLines[rank] = i;
		if (outFlags) {
			const uint32_t lane = threadIdx.x & 63;
			const uint64_t* m = marks + (i >> 6) * 2;   // (line i: wave i / 64 of the batch)
			outFlags[rank] = uint8_t(((m[0] >> lane) & 1 ? PIRE_HIP_CONTEXT_HIT : 0) | ((m[1] >> lane) & 1 ? PIRE_HIP_CONTEXT_GROUP : 0));
		}
	}
};

__global__ __launch_bounds__(kBlockThreads) void ContextClassifyKernel(ContextPass p, TileScratch t)
{
	__shared__ uint32_t waveCount[kBlockWaves];
	__shared__ uint32_t groupWave[kBlockWaves];
	__shared__ uint64_t hitWords[kBlockWaves];
	__shared__ uint64_t selWords[kBlockWaves];
	__shared__ uint64_t slice[2];
	__shared__ uint8_t mark[kBlockThreads];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t k = std::min(p.hitCount ? *p.hitCount : p.hitCap, p.hitCap);
	for (uint32_t tile = blockIdx.x; tile < t.tiles; tile += gridDim.x) {
		const uint64_t t0 = uint64_t(tile) * kBlockThreads, t1 = std::min(t0 + kBlockThreads, p.n);
		const uint64_t i = t0 + threadIdx.x;
		// the slice of the list inside the tile: hits[lo, hi)
		if (wave < 2) {
			const uint64_t at = WaveBound<false>(p.hits, k, wave ? t1 : t0);
			if (lane == 0)
				slice[wave] = at;
		}
		mark[threadIdx.x] = 0;
		__syncthreads();
		const uint64_t lo = slice[0], hi = std::max(slice[1], lo);
		if (threadIdx.x < hi - lo) {
			const uint64_t h = LoadU64(p.hits, lo + threadIdx.x);
			if (h >= t0 && h < t1)
				mark[h - t0] = 1;
		}
		__syncthreads();
		const bool hit = mark[threadIdx.x] != 0;
		const uint64_t hitBallot = __ballot(hit);
		if (lane == 0)
			hitWords[wave] = hitBallot;
		// the one entry outside the slice on either side, and the first entry not in front of the tile
		const bool havePrev = lo > 0, haveNext = hi < k, haveFirst = lo < k;
		const uint64_t prev = havePrev ? LoadU64(p.hits, lo - 1) : 0;
		const uint64_t next = haveNext ? LoadU64(p.hits, hi) : 0;
		const uint64_t first = haveFirst ? LoadU64(p.hits, lo) : 0;
		__syncthreads();
		// the nearest hit at or before the line, the nearest at or after it
		bool havePred = false, haveSucc = false;
		uint64_t pred = 0, succ = 0;
		{
			uint64_t w = hitBallot & (~0ull >> (63 - lane));
			uint32_t at = wave;
			for (uint32_t v = wave; v-- > 0 && !w;)
				if (hitWords[v])
					w = hitWords[v], at = v;
			if (w)
				havePred = true, pred = t0 + at * 64 + (63 - uint32_t(__clzll(static_cast<long long>(w))));
			else if (havePrev)
				havePred = true, pred = prev;
		}
		{
			uint64_t w = hitBallot & (~0ull << lane);
			uint32_t at = wave;
			for (uint32_t v = wave + 1; v < kBlockWaves && !w; ++v)
				if (hitWords[v])
					w = hitWords[v], at = v;
			if (w)
				haveSucc = true, succ = t0 + at * 64 + uint32_t(__ffsll(static_cast<long long>(w)) - 1);
			else if (haveNext)
				haveSucc = true, succ = next;
		}
		const bool sel = i < p.n && ((havePred && i - pred <= p.after) || (haveSucc && succ - i <= p.before));
		const uint64_t selBallot = __ballot(sel);
		if (lane == 0)
			selWords[wave] = selBallot;
		__syncthreads();
		// a run begins where the line in front is not selected
		bool front;
		if (lane)
			front = (selBallot >> (lane - 1)) & 1;
		else if (wave)
			front = selWords[wave - 1] >> 63;
		else   // line t0 - 1 lies behind every entry in front of the slice and in front of every other
			front = t0 && ((havePrev && t0 - 1 - prev <= p.after) || (haveFirst && first - (t0 - 1) <= p.before));
		const uint64_t groupBallot = __ballot(sel && !front);
		if (lane == 0) {
			groupWave[wave] = uint32_t(__popcll(groupBallot));
			uint64_t* m = p.marks + (size_t(tile) * kBlockWaves + wave) * 2;
			m[0] = hitBallot;
			m[1] = groupBallot;
		}
		TileBallot(sel, tile, t.ballots, t.tileCounts, waveCount);   // (two barriers: groupWave is whole)
		if (threadIdx.x == 0) {
			uint32_t sum = 0;
			for (uint32_t w = 0; w < kBlockWaves; ++w)
				sum += groupWave[w];
			p.groupCounts[tile] = sum;
		}
	}
}

int ZeroCounts(uint64_t* outLineCount, uint64_t* outGroupCount, hipStream_t stream)
{
	hipError_t e = hipMemsetAsync(outLineCount, 0, 8, stream);
	if (e == hipSuccess && outGroupCount)
		e = hipMemsetAsync(outGroupCount, 0, 8, stream);
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemsetAsync(line count)");
}

}  // namespace

int LaunchContext(const uint64_t* hits, const uint64_t* hitCount, uint64_t hitCap, uint64_t n, uint64_t before, uint64_t after,
                  uint64_t* outLines, uint8_t* outFlags, uint64_t lineCap, uint64_t* outLineCount, uint64_t* outGroupCount,
                  hipStream_t stream)
{
	if (n == 0 || hitCap == 0)
		return ZeroCounts(outLineCount, outGroupCount, stream);
	TilePass t(stream);
	StreamScratch marks(stream);
	const int rc = t.Front("pire_hip_context", "hipMallocAsync(context scratch)", n, outLineCount);
	if (rc || !t.s.tiles)
		return rc;
	ContextPass p;
	// 2 * n / 8 bytes of hit and run words + n / 256 bytes of run counts
	const size_t markBytes = size_t(t.s.tiles) * kBlockWaves * 16;
	if (int rc2 = marks.Alloc(markBytes + size_t(t.s.tiles) * 4, "hipMallocAsync(context marks)"))
		return rc2;
	p.marks = marks.as<uint64_t>();
	p.groupCounts = reinterpret_cast<uint32_t*>(marks.as<uint8_t>() + markBytes);
	p.hits = hits;
	p.hitCount = hitCount;
	p.hitCap = hitCap;
	p.n = n;
	p.before = before;
	p.after = after;
	p.outLines = outLines;
	p.outFlags = outLines ? outFlags : nullptr;
	hipLaunchKernelGGL(ContextClassifyKernel, t.Grid(), dim3(kBlockThreads), 0, stream, p, t.s);
	t.Scan(outLineCount);
	if (outGroupCount)
		LaunchTileScan(p.groupCounts, 1, t.s.tiles, outGroupCount, stream);
	t.Scatter(p, outLines ? lineCap : 0);
	return t.Done("context launch");
}

int ContextArgsInvalid(const char* who, bool haveHits, uint64_t hitCap, uint64_t n, const ContextOut& o, bool ownList)
{
	const char* what = !o.outLineCount                         ? "null out_line_count"
	                   : hitCap && !haveHits                   ? "hit_cap > 0 with null hits"
	                   : o.lineCap && !o.outLines && !ownList  ? "line_cap > 0 with null out_lines"
	                   : o.outFlags && !o.outLines             ? "out_line_flags without out_lines"
	                   : n >= (1ull << 32)                     ? "2^32 lines or more in one call"
	                   : hitCap >= (1ull << 32)                ? "2^32 hits or more in one call"
	                                                           : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

int ContextHitsInvalid(const char* who, const void* hits, uint64_t k, uint64_t n)
{
	const char* what = nullptr;
	uint64_t last = 0;
	for (uint64_t j = 0; j < k && !what; ++j) {
		uint64_t h;   // (`hits` may have any alignment)
		memcpy(&h, static_cast<const uint8_t*>(hits) + j * 8, 8);
		what = h >= n ? "hit out of range" : j && h <= last ? "hits must be strictly ascending" : nullptr;
		last = h;
	}
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

}  // namespace pirehip

using namespace pirehip;

extern "C" int pire_hip_context(const uint64_t* hits, const uint64_t* hit_count, uint64_t hit_cap, uint64_t n, uint64_t before,
                                uint64_t after, uint32_t flags, uint64_t* out_lines, uint8_t* out_line_flags, uint64_t line_cap,
                                uint64_t* out_line_count, uint64_t* out_group_count, void* streamPtr)
try {
	const char* who = "pire_hip_context";
	const ContextOut o = {out_lines, out_line_flags, line_cap, out_line_count, out_group_count};
	if (int rc = ContextArgsInvalid(who, hits != nullptr, hit_cap, n, o))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	if (flags & PIRE_HIP_RUN_ON_DEVICE)
		return LaunchContext(hits, hit_count, hit_cap, n, before, after, out_lines, out_line_flags, line_cap, out_line_count, out_group_count,
		                     stream);
	// host pointers: the list is looked at, staged in, the kernels, staged out -- the lists only as far as they were written
	const uint64_t k = std::min(hit_count ? *hit_count : hit_cap, hit_cap);
	if (int rc = ContextHitsInvalid(who, hits, k, n))
		return rc;
	if (n == 0 || k == 0) {
		*out_line_count = 0;
		if (out_group_count)
			*out_group_count = 0;
		return PIRE_HIP_OK;
	}
	BatchIO io(stream, false);
	const uint8_t* dHits = nullptr;
	HitStage list(false, out_line_count, "hipMemcpy(context lines)");   // n lines: no list is staged longer
	uint64_t *dGroups = nullptr, *dLines = nullptr;
	uint8_t* dFlags = nullptr;
	int rc;
	if ((rc = io.In(reinterpret_cast<const uint8_t*>(hits), size_t(k) * 8, &dHits)) || (rc = list.Count(io, line_cap, n)))
		return rc;
	if (out_group_count)
		if ((rc = io.Result(out_group_count, 1, 1, &dGroups)))
			return rc;
	if ((rc = list.List(io, out_lines, 1, &dLines)) || (rc = list.List(io, out_line_flags, 1, &dFlags)) || (rc = io.Ready()))
		return rc;
	if ((rc = LaunchContext(reinterpret_cast<const uint64_t*>(dHits), nullptr, k, n, before, after, dLines, dFlags, list.cap, list.dCount, dGroups,
	                        stream)))
		return rc;
	if ((rc = io.Finish()))
		return rc;
	return list.Back();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}
