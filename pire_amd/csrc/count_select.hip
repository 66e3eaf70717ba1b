// From counted matches to the strings that count on the device (pire_hip_count_select): which strings reached their
// thresholds, and how many occurrences the batch holds.
//
// pire_hip_counting_run and pire_hip_run_half_final answer with one row of R counters per string.  What a caller of a
// counting scanner wants is the strings whose counters reach a threshold -- a compacted, ascending list of their indices and
// rows -- and the occurrences of every regexp over the batch.  This unit turns the one into the other without leaving the
// device, behind ANY of the counting kernels (it reads result rows, nothing else of a scan; include/pire_hip.h has the formulas):
//
//   classify  one lane per string: its R counters against the R thresholds -> selected?  The selected bits of a wave are one
//             ballot word, kept in scratch; one count per tile of 1 024 strings.  Where totals are asked for, every counter
//             is summed over the wave by shuffles and over the tile through LDS, 16 regexps a step: one uint64 per tile and
//             regexp (a tile of 1 024 counters of 32 bits does not fit 32 bits).
//   scan      exclusive scan of the tile counts, one block; the total is the hit count (select.hip's kernel, LaunchTileScan).
//   totals    where asked for: a block per regexp adds up that regexp's tile sums -- written, not accumulated.
//   scatter   rank of a selected string = tile offset + the popcounts of the waves in front + mbcnt of its own wave's
//             ballot word; the lane writes its index and copies its row.
//
// The scatter kernel and the launcher are tile_pass.h's, the staging of the count and the lists is internal.h's HitStage; the
// classify kernel -- it ends in compact.h's TileBallot -- and its sums are this unit's own.  Launches on the caller's stream,
// the shape of select.hip: no block waits for another block, no atomics (the same input gives the same bits).  Plain HIP
// with compiler-placed waits: nothing here keeps data on its way in registers.  A row is read with 4-byte loads: `results`
// is only 4-byte aligned.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "tile_pass.h"

namespace pirehip {

namespace {

constexpr uint32_t kCntChunk = 16;                // regexps summed between two barriers: 16 waves x 16 sums of LDS
constexpr uint32_t kCntTotalBlocks = 1024;        // the totals' grid: a block per regexp, regexps in a grid-stride loop
constexpr uint32_t kCntMaxRegexps = 1024;

struct CountPass {
	const uint32_t* results;   // [n][regexps]
	uint64_t n;
	uint32_t regexps;
	const uint32_t* minCount;  // nullable: 1 for every regexp
	uint32_t all;              // PIRE_HIP_COUNT_ALL
	uint64_t* outHits;         // nullable
	uint32_t* outHitResults;   // nullable
	uint64_t* tileSums;        // [regexps][tiles] the counters of a tile added up (kSums)

	__device__ __forceinline__ void Write(uint64_t rank, uint64_t i) const
	{
		if (outHits)
			outHits[rank] = i;
		if (outHitResults) {
			const uint32_t* row = results + i * regexps;
			uint32_t* out = outHitResults + rank * regexps;
			for (uint32_t r = 0; r < regexps; ++r)
				out[r] = row[r];
		}
	}
};

template <bool kSums>
__global__ __launch_bounds__(kBlockThreads) void CountClassifyKernel(CountPass p, TileScratch t)
{
	__shared__ uint32_t waveCount[kBlockWaves];
	__shared__ uint64_t waveSum[kSums ? kBlockWaves * kCntChunk : 1];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint32_t tile = blockIdx.x; tile < t.tiles; tile += gridDim.x) {
		const uint64_t i = uint64_t(tile) * kBlockThreads + threadIdx.x;
		const bool live = i < p.n;
		const uint32_t* row = p.results + (live ? i : 0) * p.regexps;
		bool wanted = false, any = false, every = true;
		for (uint32_t r0 = 0; r0 < p.regexps; r0 += kCntChunk) {
			const uint32_t cnt = std::min(kCntChunk, p.regexps - r0);
			for (uint32_t k = 0; k < cnt; ++k) {
				const uint32_t c = live ? row[r0 + k] : 0;
				const uint32_t m = p.minCount ? p.minCount[r0 + k] : 1;
				if (m) {   // (wanted: the same for every lane)
					wanted = true;
					any = any || c >= m;
					every = every && c >= m;
				}
				if (kSums) {
					unsigned long long s = c;
					for (uint32_t d = 32; d; d >>= 1)
						s += __shfl_xor(s, int(d), 64);
					if (lane == 0)
						waveSum[wave * kCntChunk + k] = s;
				}
			}
			if (kSums) {
				__syncthreads();
				if (threadIdx.x < cnt) {
					uint64_t s = 0;
					for (uint32_t w = 0; w < kBlockWaves; ++w)
						s += waveSum[w * kCntChunk + threadIdx.x];
					p.tileSums[size_t(r0 + threadIdx.x) * t.tiles + tile] = s;
				}
				__syncthreads();   // (the next step writes waveSum again)
			}
		}
		TileBallot(live && wanted && (p.all ? every : any), tile, t.ballots, t.tileCounts, waveCount);
	}
}

__global__ __launch_bounds__(kBlockThreads) void CountTotalsKernel(const uint64_t* tileSums, uint32_t regexps, uint32_t tiles, uint64_t* outTotals)
{
	__shared__ uint64_t waveSum[kBlockWaves];
	for (uint32_t r = blockIdx.x; r < regexps; r += gridDim.x) {
		const uint64_t* row = tileSums + size_t(r) * tiles;
		uint64_t s = 0;
		for (uint32_t t = threadIdx.x; t < tiles; t += kBlockThreads)
			s += row[t];
		uint64_t total;
		(void)BlockExclusive(s, waveSum, &total);
		if (threadIdx.x == 0)
			outTotals[r] = total;   // n < 2^32 counters of 32 bits: the sum fits
	}
}

}  // namespace

int LaunchCountSelect(const uint32_t* results, uint64_t n, uint32_t regexps, const uint32_t* minCount, uint32_t mode, uint64_t* outTotals,
                      uint64_t* outHits, uint32_t* outHitResults, uint64_t hitCap, uint64_t* outHitCount, hipStream_t stream)
{
	if (regexps == 0)
		n = 0;   // no regexp is wanted: a count of 0, nothing else
	if (n == 0 && outTotals && regexps) {
		const hipError_t e = hipMemsetAsync(outTotals, 0, size_t(regexps) * 8, stream);
		if (e != hipSuccess)
			return HipFail(e, "hipMemsetAsync(totals)");
	}
	TilePass t(stream);
	StreamScratch sums(stream);
	const int rc = t.Front("pire_hip_count_select", "hipMallocAsync(count select scratch)", n, outHitCount);
	if (rc || !t.s.tiles)
		return rc;
	CountPass p;
	p.tileSums = nullptr;
	if (outTotals) {
		if (int src = sums.Alloc(size_t(regexps) * t.s.tiles * 8, "hipMallocAsync(count select sums)"))
			return src;
		p.tileSums = sums.as<uint64_t>();
	}
	p.results = results;
	p.n = n;
	p.regexps = regexps;
	p.minCount = minCount;
	p.all = (mode & PIRE_HIP_COUNT_ALL) != 0;
	p.outHits = outHits;
	p.outHitResults = outHitResults;
	if (outTotals) {
		hipLaunchKernelGGL(CountClassifyKernel<true>, t.Grid(), dim3(kBlockThreads), 0, stream, p, t.s);
		hipLaunchKernelGGL(CountTotalsKernel, dim3(std::min(regexps, kCntTotalBlocks)), dim3(kBlockThreads), 0, stream, p.tileSums, regexps, t.s.tiles,
		                   outTotals);
	} else {
		hipLaunchKernelGGL(CountClassifyKernel<false>, t.Grid(), dim3(kBlockThreads), 0, stream, p, t.s);
	}
	return t.Tail(p, outHits || outHitResults ? hitCap : 0, outHitCount, "count select launch");
}

int CountSelectArgsInvalid(const char* who, uint64_t n, uint32_t regexps, bool haveResults, const CountSelectOut& o)
{
	const char* what = !o.outHitCount                                       ? "null out_hit_count"
	                   : n && regexps && !haveResults                       ? "n > 0 with null results"
	                   : o.mode & ~uint32_t(PIRE_HIP_COUNT_ALL)             ? "unknown bits in mode"
	                   : o.hitCap && !o.outHits && !o.outHitResults         ? "hit_cap > 0 with null out_hits and null out_hit_results"
	                                                                        : nullptr;
	const char* unsupported = n >= (1ull << 32)         ? "2^32 strings or more in one call"
	                          : regexps > kCntMaxRegexps ? "more than 1024 regexps"
	                                                     : nullptr;
	if (!what && !unsupported)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + (what ? what : unsupported));
	return what ? PIRE_HIP_EINVAL : PIRE_HIP_EUNSUPPORTED;
}

int CountSelectStage::Empty(hipStream_t stream)
{
	if (list.onDevice)
		return LaunchCountSelect(nullptr, 0, regexps, nullptr, 0, o.outTotals, nullptr, nullptr, 0, o.outHitCount, stream);
	*o.outHitCount = 0;
	if (o.outTotals)
		std::fill(o.outTotals, o.outTotals + regexps, uint64_t(0));
	return PIRE_HIP_OK;
}

int CountSelectStage::In(BatchIO& io)
{
	return o.minCount ? io.In(o.minCount, size_t(regexps), &dMin) : PIRE_HIP_OK;
}

int CountSelectStage::Results(BatchIO& io, uint64_t n)
{
	if (int rc = list.Count(io, o.hitCap, n))
		return rc;
	if (o.outTotals && regexps)
		if (int rc = io.Result(o.outTotals, size_t(regexps), size_t(regexps), &dTotals))
			return rc;
	if (int rc = list.List(io, o.outHits, 1, &dHits))
		return rc;
	return list.List(io, o.outHitResults, regexps, &dHitResults);
}

int CountSelectStage::Launch(const uint32_t* results, uint64_t n, hipStream_t stream)
{
	return LaunchCountSelect(results, n, regexps, dMin, o.mode, dTotals, dHits, dHitResults, list.cap, list.dCount, stream);
}

}  // namespace pirehip

using namespace pirehip;

extern "C" int pire_hip_count_select(const uint32_t* results, uint64_t n, uint32_t regexps, const uint32_t* min_count, uint32_t mode,
                                     uint32_t flags, uint64_t* out_totals, uint64_t* out_hits, uint32_t* out_hit_results, uint64_t hit_cap,
                                     uint64_t* out_hit_count, void* streamPtr)
try {
	const CountSelectOut o = {min_count, mode, out_totals, out_hits, out_hit_results, hit_cap, out_hit_count};
	if (int rc = CountSelectArgsInvalid("pire_hip_count_select", n, regexps, results != nullptr, o))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	CountSelectStage pass(o, regexps, onDevice);
	if (n == 0 || regexps == 0)   // (no regexps: a count of 0 and nothing else)
		return pass.Empty(stream);
	// host pointers: staged in, the kernels, staged out -- the lists only as far as they were written
	BatchIO io(stream, onDevice);
	const uint32_t* dResults = nullptr;
	int rc;
	if ((rc = io.In(results, size_t(n) * regexps, &dResults)) || (rc = pass.In(io)) || (rc = pass.Results(io, n)) || (rc = io.Ready()))
		return rc;
	if ((rc = pass.Launch(dResults, n, stream)))
		return rc;
	if ((rc = io.Finish()))
		return rc;
	return pass.Back();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}
