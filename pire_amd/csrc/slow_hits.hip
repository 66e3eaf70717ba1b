// From Final flags to the strings that matched -- or did not -- on the device (pire_hip_final_select).
//
// pire_hip_slow_run answers with one Final byte per string and nothing else: a SlowScanner's state is a set of NFA states,
// there is no state index for pire_hip_select to look up.  What its caller wants is what every other scanner's caller
// wants: a compacted, ascending list of the strings that matched -- or, for `grep -v`, of those that did not.  This unit
// turns the one into the other without leaving the device.  It takes no table: it reads flag bytes, whoever wrote them
// (out_final of pire_hip_run and pire_hip_run_pair as well: a flag counts as set when it is not 0).
//
//   classify  one lane per string: (final[i] != 0) != invert -> selected?  The selected bits of a wave are one ballot word,
//             kept in scratch; one count per tile of 1 024 strings.
//   scan      exclusive scan of the tile counts, one block; the total is the hit count (select.hip's kernel, LaunchTileScan).
//   scatter   rank of a selected string = tile offset + the popcounts of the waves in front + mbcnt of its own wave's
//             ballot word; the lane writes its index.
//
// The classify tail, the scatter head and the launcher's front are the select pass's (compact.h TileBallot / TileRank,
// select.hip TileCompaction); this unit keeps its predicate and what a selected lane writes.  Launches on the caller's
// stream, the shape of select.hip: no block waits for another block, no atomics (the same input gives the same bits).
// Plain HIP with compiler-placed waits: nothing here keeps data on its way in registers.  A flag is read with a byte load
// (a wave reads 64 consecutive bytes, a tile 1 KiB): `final` may have any alignment.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "compact.h"
#include "internal.h"

namespace pirehip {

namespace {

constexpr uint32_t kFinThreads = kBlockThreads;   // one tile = 1 024 strings = 16 ballot words
constexpr uint32_t kFinWaves = kBlockWaves;
constexpr uint32_t kFinMaxBlocks = 8192;

struct FinalSelectParams {
	const uint8_t* fin;     // [n]
	uint64_t n;
	uint32_t invert;        // PIRE_HIP_FINAL_SELECT_ZERO
	uint64_t* outHits;
	uint64_t hitCap;
	uint64_t* ballots;      // [tiles * 16] selected bits, one word per wave
	uint32_t* tileCounts;   // [tiles] selected strings per tile; after the scan: selected strings in front of the tile
	uint32_t tiles;
};

__global__ __launch_bounds__(kFinThreads) void FinalClassifyKernel(FinalSelectParams p)
{
	__shared__ uint32_t waveCount[kFinWaves];
	for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
		const uint64_t i = uint64_t(tile) * kFinThreads + threadIdx.x;
		const bool live = i < p.n;
		const bool set = live && p.fin[i] != 0;
		TileBallot(live && set != (p.invert != 0), tile, p.ballots, p.tileCounts, waveCount);
	}
}

__global__ __launch_bounds__(kFinThreads) void FinalScatterKernel(FinalSelectParams p)
{
	for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
		bool selected;
		const uint64_t rank = TileRank(tile, p.ballots, p.tileCounts, &selected);
		if (selected && rank < p.hitCap)   // (a selected bit: i < n)
			p.outHits[rank] = uint64_t(tile) * kFinThreads + threadIdx.x;
	}
}

}  // namespace

int LaunchFinalSelect(const uint8_t* fin, uint64_t n, uint32_t mode, uint64_t* outHits, uint64_t hitCap, uint64_t* outHitCount,
                      hipStream_t stream)
{
	FinalSelectParams p;
	StreamScratch scratch(stream);
	const int rc = TileCompaction("pire_hip_final_select", "hipMallocAsync(final select scratch)", n, outHitCount, stream, scratch, &p.tiles,
	                              &p.ballots, &p.tileCounts);
	if (rc || !p.tiles)
		return rc;
	p.fin = fin;
	p.n = n;
	p.invert = mode == PIRE_HIP_FINAL_SELECT_ZERO;
	p.outHits = outHits;
	p.hitCap = outHits ? hitCap : 0;
	const dim3 grid(std::min(p.tiles, kFinMaxBlocks));
	hipLaunchKernelGGL(FinalClassifyKernel, grid, dim3(kFinThreads), 0, stream, p);
	LaunchTileScan(p.tileCounts, 1, p.tiles, outHitCount, stream);
	if (p.hitCap)
		hipLaunchKernelGGL(FinalScatterKernel, grid, dim3(kFinThreads), 0, stream, p);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "final select launch");
}

int FinalSelectArgsInvalid(const char* who, uint64_t n, bool haveFinal, const FinalSelectOut& o)
{
	const char* what = o.mode > PIRE_HIP_FINAL_SELECT_ZERO  ? "unknown mode"
	                   : !o.outHitCount                     ? "null out_hit_count"
	                   : n && !haveFinal                    ? "n > 0 with null final"
	                   : o.hitCap && !o.outHits             ? "hit_cap > 0 with null out_hits"
	                   : n >= (1ull << 32)                  ? "2^32 strings or more in one call"
	                                                        : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

int FinalSelectStage::Empty(hipStream_t stream)
{
	if (onDevice)
		return LaunchFinalSelect(nullptr, 0, o.mode, nullptr, 0, o.outHitCount, stream);
	*o.outHitCount = 0;
	return PIRE_HIP_OK;
}

int FinalSelectStage::Results(BatchIO& io, uint64_t n)
{
	cap = onDevice ? o.hitCap : std::min<uint64_t>(o.hitCap, n);   // n strings have at most n hits: a host call stages no more
	if (int rc = io.Result(onDevice ? o.outHitCount : &count, 1, 1, &dCount))   // (host pointers: the count comes back here first)
		return rc;
	if (o.outHits && cap)
		if (int rc = io.Result(o.outHits, size_t(cap), 0, &dHits))
			return rc;
	return PIRE_HIP_OK;
}

int FinalSelectStage::Launch(const uint8_t* fin, uint64_t n, hipStream_t stream)
{
	return LaunchFinalSelect(fin, n, o.mode, dHits, cap, dCount, stream);
}

int FinalSelectStage::Back()
{
	if (onDevice)
		return PIRE_HIP_OK;
	*o.outHitCount = count;
	const uint64_t written = std::min<uint64_t>(count, cap);
	const hipError_t e = written && dHits ? hipMemcpy(o.outHits, dHits, size_t(written) * 8, hipMemcpyDeviceToHost) : hipSuccess;
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemcpy(hits)");
}

}  // namespace pirehip

using namespace pirehip;

extern "C" int pire_hip_final_select(const uint8_t* final, uint64_t n, uint32_t mode, uint32_t flags, uint64_t* out_hits, uint64_t hit_cap,
                                     uint64_t* out_hit_count, void* streamPtr)
try {
	const FinalSelectOut o = {mode, out_hits, hit_cap, out_hit_count};
	if (int rc = FinalSelectArgsInvalid("pire_hip_final_select", n, final != nullptr, o))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	FinalSelectStage pass(o, onDevice);
	if (n == 0)
		return pass.Empty(stream);
	// host pointers: staged in, the kernels, staged out -- the list only as far as it was written
	BatchIO io(stream, onDevice);
	const uint8_t* dFinal = nullptr;
	int rc;
	if ((rc = io.In(final, size_t(n), &dFinal)) || (rc = pass.Results(io, n)) || (rc = io.Ready()))
		return rc;
	if ((rc = pass.Launch(dFinal, n, stream)))
		return rc;
	if ((rc = io.Finish()))
		return rc;
	return pass.Back();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}
