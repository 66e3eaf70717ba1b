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
// The classify tail, the scatter head and the launcher's front are the select pass's (compact.h TileBallot / TileRank,
// select.hip TileCompaction); this unit keeps its predicate and what a selected lane writes.  Launches on the caller's
// stream: no block waits for another block, no atomics (the same input gives the same bits).  Plain HIP with
// compiler-placed waits: nothing here keeps data on its way in registers.  `hits` may have any alignment: an entry is read
// through a packed type.  A list that is not ascending or names lines >= n gives an unspecified selection and nothing worse:
// every index into `hits` is clamped into [0, k), every index into the tile's bytes is checked against the tile.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "compact.h"
#include "internal.h"

namespace pirehip {

namespace {

constexpr uint32_t kCtxThreads = kBlockThreads;   // one tile = 1 024 lines = 16 ballot words
constexpr uint32_t kCtxWaves = kBlockWaves;
constexpr uint32_t kCtxMaxBlocks = 8192;

struct __attribute__((packed, aligned(1))) UnalignedU64 {
	uint64_t v;
};

struct ContextParams {
	const uint64_t* hits;       // [k], any alignment
	const uint64_t* hitCount;   // nullable: k = hitCap
	uint64_t hitCap;
	uint64_t n;
	uint64_t before, after;
	uint64_t* outLines;         // nullable
	uint8_t* outFlags;          // nullable
	uint64_t lineCap;
	uint64_t* ballots;          // [tiles * 16] selected bits, one word per wave
	uint32_t* tileCounts;       // [tiles] selected lines per tile; after the scan: selected lines in front of the tile
	uint64_t* marks;            // [tiles * 16][2] hit bits and run bits of the wave
	uint32_t* groupCounts;      // [tiles] runs that begin in the tile
	uint32_t tiles;
};

__device__ __forceinline__ uint64_t HitAt(const uint64_t* hits, uint64_t j)
{
	return reinterpret_cast<const UnalignedU64*>(hits)[j].v;
}

// How many of hits[0, k) are < x (the list ascends), found by one wave: 64 probes a step, every probe inside [0, k)
__device__ __forceinline__ uint64_t WaveLowerBound(const uint64_t* hits, uint64_t k, uint64_t x)
{
	const uint32_t lane = threadIdx.x & 63;
	uint64_t lo = 0, hi = k;   // the answer is in [lo, hi]
	while (hi > lo) {
		const uint64_t step = (hi - lo + 63) / 64;
		const uint64_t q = lo + (lane + 1) * step - 1;
		const bool lt = q < hi && HitAt(hits, q) < x;   // true in the first c lanes, false behind them
		const uint64_t c = uint64_t(__popcll(__ballot(lt)));
		hi = std::min(hi, lo + (c + 1) * step - 1);
		lo = std::min(lo + c * step, hi);   // (the min: a list that does not ascend)
	}
	return lo;
}

__global__ __launch_bounds__(kCtxThreads) void ContextClassifyKernel(ContextParams p)
{
	__shared__ uint32_t waveCount[kCtxWaves];
	__shared__ uint32_t groupWave[kCtxWaves];
	__shared__ uint64_t hitWords[kCtxWaves];
	__shared__ uint64_t selWords[kCtxWaves];
	__shared__ uint64_t slice[2];
	__shared__ uint8_t mark[kCtxThreads];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t k = std::min(p.hitCount ? *p.hitCount : p.hitCap, p.hitCap);
	for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
		const uint64_t t0 = uint64_t(tile) * kCtxThreads, t1 = std::min(t0 + kCtxThreads, p.n);
		const uint64_t i = t0 + threadIdx.x;
		// the slice of the list inside the tile: hits[lo, hi)
		if (wave < 2) {
			const uint64_t at = WaveLowerBound(p.hits, k, wave ? t1 : t0);
			if (lane == 0)
				slice[wave] = at;
		}
		mark[threadIdx.x] = 0;
		__syncthreads();
		const uint64_t lo = slice[0], hi = std::max(slice[1], lo);
		if (threadIdx.x < hi - lo) {
			const uint64_t h = HitAt(p.hits, lo + threadIdx.x);
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
		const uint64_t prev = havePrev ? HitAt(p.hits, lo - 1) : 0;
		const uint64_t next = haveNext ? HitAt(p.hits, hi) : 0;
		const uint64_t first = haveFirst ? HitAt(p.hits, lo) : 0;
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
			for (uint32_t v = wave + 1; v < kCtxWaves && !w; ++v)
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
			uint64_t* m = p.marks + (size_t(tile) * kCtxWaves + wave) * 2;
			m[0] = hitBallot;
			m[1] = groupBallot;
		}
		TileBallot(sel, tile, p.ballots, p.tileCounts, waveCount);   // (two barriers: groupWave is whole)
		if (threadIdx.x == 0) {
			uint32_t sum = 0;
			for (uint32_t w = 0; w < kCtxWaves; ++w)
				sum += groupWave[w];
			p.groupCounts[tile] = sum;
		}
	}
}

__global__ __launch_bounds__(kCtxThreads) void ContextScatterKernel(ContextParams p)
{
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
		bool selected;
		const uint64_t rank = TileRank(tile, p.ballots, p.tileCounts, &selected);
		if (selected && rank < p.lineCap) {   // (a selected bit: i < n)
			p.outLines[rank] = uint64_t(tile) * kCtxThreads + threadIdx.x;
			if (p.outFlags) {
				const uint64_t* m = p.marks + (size_t(tile) * kCtxWaves + wave) * 2;
				p.outFlags[rank] = uint8_t(((m[0] >> lane) & 1 ? PIRE_HIP_CONTEXT_HIT : 0) | ((m[1] >> lane) & 1 ? PIRE_HIP_CONTEXT_GROUP : 0));
			}
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
	ContextParams p;
	StreamScratch scratch(stream), marks(stream);
	const int rc = TileCompaction("pire_hip_context", "hipMallocAsync(context scratch)", n, outLineCount, stream, scratch, &p.tiles, &p.ballots,
	                              &p.tileCounts);
	if (rc || !p.tiles)
		return rc;
	// 2 * n / 8 bytes of hit and run words + n / 256 bytes of run counts
	const size_t markBytes = size_t(p.tiles) * kCtxWaves * 16;
	if (int rc2 = marks.Alloc(markBytes + size_t(p.tiles) * 4, "hipMallocAsync(context marks)"))
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
	p.lineCap = outLines ? lineCap : 0;
	const dim3 grid(std::min(p.tiles, kCtxMaxBlocks));
	hipLaunchKernelGGL(ContextClassifyKernel, grid, dim3(kCtxThreads), 0, stream, p);
	LaunchTileScan(p.tileCounts, 1, p.tiles, outLineCount, stream);
	if (outGroupCount)
		LaunchTileScan(p.groupCounts, 1, p.tiles, outGroupCount, stream);
	if (p.lineCap)
		hipLaunchKernelGGL(ContextScatterKernel, grid, dim3(kCtxThreads), 0, stream, p);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "context launch");
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
	uint64_t count = 0;   // the count comes back here first
	uint64_t *dCount = nullptr, *dGroups = nullptr, *dLines = nullptr;
	uint8_t* dFlags = nullptr;
	const uint64_t cap = std::min(line_cap, n);   // n lines: no list is staged longer
	int rc;
	if ((rc = io.In(reinterpret_cast<const uint8_t*>(hits), size_t(k) * 8, &dHits)) || (rc = io.Result(&count, 1, 1, &dCount)))
		return rc;
	if (out_group_count)
		if ((rc = io.Result(out_group_count, 1, 1, &dGroups)))
			return rc;
	if (out_lines && cap)
		if ((rc = io.Result(out_lines, size_t(cap), 0, &dLines)))
			return rc;
	if (out_line_flags && cap)
		if ((rc = io.Result(out_line_flags, size_t(cap), 0, &dFlags)))
			return rc;
	if ((rc = io.Ready()))
		return rc;
	if ((rc = LaunchContext(reinterpret_cast<const uint64_t*>(dHits), nullptr, k, n, before, after, dLines, dFlags, cap, dCount, dGroups, stream)))
		return rc;
	if ((rc = io.Finish()))
		return rc;
	*out_line_count = count;
	const uint64_t written = std::min(count, cap);
	hipError_t e = hipSuccess;
	if (written && dLines)
		e = hipMemcpy(out_lines, dLines, size_t(written) * 8, hipMemcpyDeviceToHost);
	if (e == hipSuccess && written && dFlags)
		e = hipMemcpy(out_line_flags, dFlags, size_t(written), hipMemcpyDeviceToHost);
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemcpy(context lines)");
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}
