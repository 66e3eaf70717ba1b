// Every leftmost-longest match of every string (pire_hip_search_all): search.hip's two reference searches, iterated.
//
//   p = 0
//   while p < len:
//       t = LongestSuffix(R, string from p)          t <= 0: stop                                      run.h:313-341
//       b = len - t
//       h = LongestPrefix(F, string from b)          (ShortestPrefix where asked for)  h < 0: stop     run.h:277-311
//       h > 0: a match, [b, b + h)                   p = b + max(h, 1)              (include/pire_hip.h has the formulas)
//
// R's state after the bytes len-1 .. j does not depend on p, so ONE backward walk answers every LongestSuffix of the loop:
//   LongestSuffix(R, string from p) = len - min{ j >= p : mark(j) }
//   mark(j) = Final(state after byte j) || (j == 0 && B && Final(Step(that state, BeginMark)))      none below a Dead state
// The marks are one bit per byte of the text, kept in stream-ordered scratch as one 16-bit word per 16-byte block of the
// text's ADDRESS: the word of block a of string i is marks[a - (text >> 4) + i].  The `+ i` gives two strings that share a
// block words of their own, so no lane writes a word that another lane reads or writes: no atomics, and the same input gives
// the same bits.  A lane writes the word of EVERY block that holds a byte of its string -- zero below the position where its
// walk met a Dead state --, so a word it reads is one it wrote in this call: nothing of an earlier call in the same scratch
// is ever read, and the scratch is not cleared.
//
// Four launches on the caller's stream, one string per lane, 1 024-thread blocks, tables in LDS as search.hip has them:
//   mark + count  the backward walk through R (exact.hip's suffix walk, recording instead of remembering one position), then
//                 the forward loop over the marks: next mark >= p, PrefixWalk through F from there.  counts[i].
//   rows          exclusive 64-bit scan of the counts (compact.h's BlockExclusive per tile of 1 024, tile sums, a scan of the
//                 tile sums by one block); the total is the match count.
//   fill          the forward loop again, F only: owners and spans into [rows[i], rows[i+1]) below the capacity.
// The parameters, the marks and the forward loop are in match_loop.h: lex.hip walks the same loop and labels what it finds.
// Plain HIP with compiler-placed waits: nothing here keeps data on its way in registers.

#include "device_common.h"
#include "walk.h"
#include "compact.h"
#include "match_loop.h"

namespace pirehip {

namespace {

// The forward leg of MatchLoop (match_loop.h): LongestPrefix / ShortestPrefix through F, its dense rows at ldsF
__device__ __forceinline__ auto ForwardLeg(const SearchAllParams& q, const uint8_t* ldsF, const LdsLayout& LF)
{
	return [&q, ldsF, &LF](const uint8_t* text, uint64_t len, uint32_t st) {
		return PrefixWalk(q.fwd, ldsF, LF, text, len, st, q.longest, q.throughEnd);
	};
}

__global__ __launch_bounds__(1024) void SearchAllMarkKernel(SearchAllParams q)
{
	const ScanParams& pr = q.rev;
	const ScanParams& pf = q.fwd;
	extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
	const LdsLayout LR = MakeLayout(pr.hot, 0, kRotPitch, 0);
	const LdsLayout LF = MakeLayout(pf.hot, 0, kRotPitch, 0);
	uint8_t* ldsF = lds + LR.total;   // (a layout's total is a multiple of 16)
	LoadTableToLds(pr, lds, LR);
	LoadTableToLds(pf, ldsF, LF);
	const uint64_t n = pr.n;
	for (uint64_t s = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < n; s += uint64_t(gridDim.x) * blockDim.x) {
		uint64_t b, len;
		StringOf(q, s, &b, &len);
		uint64_t count = 0;
		if (len) {
			const uint64_t lo = reinterpret_cast<uint64_t>(pr.text) + b;
			MarkWalk(q, lds, LR, s, lo, lo + len);
			count = MatchLoop(q, s, b, len, ~uint64_t(0), ForwardLeg(q, ldsF, LF), [](uint64_t, uint64_t, uint64_t) {});
		}
		q.counts[s] = count;
	}
}

// rows[i] = the matches in front of string i inside its tile of 1 024 strings; tileSums[tile] = the matches of the tile
__global__ __launch_bounds__(1024) void SearchAllTileKernel(SearchAllParams q, uint32_t tiles)
{
	__shared__ uint64_t waveSum[kBlockWaves];
	const uint64_t n = q.rev.n;
	for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
		const uint64_t s = uint64_t(tile) * kBlockThreads + threadIdx.x;
		const uint64_t v = s < n ? q.counts[s] : 0;
		uint64_t total;
		const uint64_t before = BlockExclusive(v, waveSum, &total);
		if (s < n)
			q.rows[s] = before;
		if (threadIdx.x == 0)
			q.tileSums[tile] = total;
	}
}

// One block: the exclusive scan of the tile sums in place; the total is rows[n] and the match count
__global__ __launch_bounds__(1024) void SearchAllSumKernel(SearchAllParams q, uint32_t tiles)
{
	__shared__ uint64_t waveSum[kBlockWaves];
	uint64_t carry = 0;
	for (uint32_t base = 0; base < tiles; base += kBlockThreads) {
		const uint32_t t = base + threadIdx.x;
		const uint64_t v = t < tiles ? q.tileSums[t] : 0;
		uint64_t total;
		const uint64_t before = BlockExclusive(v, waveSum, &total);
		if (t < tiles)
			q.tileSums[t] = carry + before;
		carry += total;
	}
	if (threadIdx.x == 0) {
		q.rows[q.rev.n] = carry;
		*q.outCount = carry;
	}
}

// lists != 0: the forward loop again, into the lists.  rows[i] becomes the matches in front of string i in the batch.
__global__ __launch_bounds__(1024) void SearchAllFillKernel(SearchAllParams q, uint32_t lists)
{
	const ScanParams& pf = q.fwd;
	extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
	const LdsLayout LF = MakeLayout(pf.hot, 0, kRotPitch, 0);
	if (lists)
		LoadTableToLds(pf, lds, LF);
	const uint64_t n = q.rev.n;
	for (uint64_t s = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < n; s += uint64_t(gridDim.x) * blockDim.x) {
		const uint64_t row = q.rows[s] + q.tileSums[s / kBlockThreads];
		q.rows[s] = row;
		if (!lists || row >= q.cap)
			continue;
		const uint64_t count = q.counts[s];
		if (!count)
			continue;
		const uint64_t room = q.cap - row;
		uint64_t b, len;
		StringOf(q, s, &b, &len);
		const uint64_t base = b + q.shift * s;
		MatchLoop(q, s, b, len, count < room ? count : room, ForwardLeg(q, lds, LF), [&](uint64_t k, uint64_t begin, uint64_t end) {
			if (q.outOwners)
				q.outOwners[row + k] = s;
			if (q.outSpans) {
				q.outSpans[2 * (row + k)] = base + begin;
				q.outSpans[2 * (row + k) + 1] = base + end;
			}
		});
	}
}

}  // namespace

int LaunchSearchAllRows(const SearchAllParams& q, uint32_t tiles, hipStream_t stream)
{
	hipLaunchKernelGGL(SearchAllTileKernel, dim3(std::min(tiles, kTileMaxBlocks)), dim3(kBlockThreads), 0, stream, q, tiles);
	hipLaunchKernelGGL(SearchAllSumKernel, dim3(1), dim3(kBlockThreads), 0, stream, q, tiles);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "search rows launch");
}

int LaunchSearchAll(const ScanParams& rev, const ScanParams& fwd, uint32_t fwdStartBegin, uint32_t opts, uint64_t textBytes, uint64_t shift,
                    uint64_t* outRows, uint64_t* outOwners, uint64_t* outSpans, uint64_t cap, uint64_t* outCount, hipStream_t stream)
{
	const uint64_t n = rev.n;
	if (n == 0) {
		hipError_t e = hipMemsetAsync(outCount, 0, 8, stream);
		if (e == hipSuccess && outRows)
			e = hipMemsetAsync(outRows, 0, 8, stream);
		return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemsetAsync(match count)");
	}
	SearchAllParams q;
	q.rev = rev;
	q.fwd = fwd;
	q.rev.compact = q.fwd.compact = 0;   // the dense rows only: no room for the warm rows of two tables
	q.fwd.n = n;
	q.fwd.text = rev.text;
	q.fwd.offsets = rev.offsets;
	q.fwdStartBegin = fwdStartBegin;
	q.longest = (opts & PIRE_HIP_SEARCH_SHORTEST) ? 0 : 1;
	q.throughBegin = (opts & PIRE_HIP_SEARCH_THROUGH_BEGIN) ? 1 : 0;
	q.throughEnd = (opts & PIRE_HIP_SEARCH_THROUGH_END) ? 1 : 0;
	q.textBytes = textBytes;
	q.shift = shift;
	q.outOwners = cap ? outOwners : nullptr;
	q.outSpans = cap ? outSpans : nullptr;
	q.cap = cap;
	q.outCount = outCount;
	int cus = 0, dev = 0;
	if (int rc = DeviceCUs(&cus, &dev))
		return rc;
	const uint32_t ldsF = MakeLayout(fwd.hot, 0, kRotPitch, 0).total;
	const uint32_t ldsBytes = MakeLayout(rev.hot, 0, kRotPitch, 0).total + ldsF;
	int limit = 0;
	hipError_t e = hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
	if (e != hipSuccess)
		return HipFail(e, "hipDeviceGetAttribute(LDS per block)");
	if (ldsBytes > uint32_t(limit)) {
		SetError("pire_hip_search_all: the two tables' dense rows take " + std::to_string(ldsBytes) + " bytes of LDS, the device has " +
		         std::to_string(limit) + " per block");
		return PIRE_HIP_EUNSUPPORTED;
	}
	// one block of scratch: counts[n], tile sums, rows[n + 1] where the caller has no array for them, the marks
	const uint32_t tiles = uint32_t((n + kBlockThreads - 1) / kBlockThreads);
	const size_t markWords = size_t(textBytes / 16) + size_t(n) + 2;
	const size_t words64 = size_t(n) + tiles + (outRows ? 0 : size_t(n) + 1);
	StreamScratch scratch(stream);
	if (int rc = scratch.Alloc(words64 * 8 + markWords * 2, "hipMallocAsync(search marks)"))
		return rc;
	q.counts = scratch.as<uint64_t>();
	q.tileSums = q.counts + n;
	q.rows = outRows ? outRows : q.tileSums + tiles;
	q.marks = reinterpret_cast<uint16_t*>(scratch.as<uint64_t>() + words64);
	const unsigned threads = kBlockThreads;
	const unsigned blocks = unsigned(std::max<uint64_t>(1, std::min<uint64_t>(tiles, uint64_t(cus) * 2)));
	if (int rc = Launch(SearchAllMarkKernel, blocks, threads, ldsBytes, stream, "search marks launch", q))
		return rc;
	if (int rc = LaunchSearchAllRows(q, tiles, stream))
		return rc;
	const uint32_t lists = q.outOwners || q.outSpans ? 1 : 0;
	if (!lists && !outRows)
		return PIRE_HIP_OK;   // the count alone
	return Launch(SearchAllFillKernel, blocks, threads, lists ? ldsF : 0, stream, "search fill launch", q, lists);
}

}  // namespace pirehip
