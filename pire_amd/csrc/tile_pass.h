// What the eight ballot compactions share around compact.h's TileBallot and TileRank (select.hip, capture_select.hip,
// count_select.hip, slow_hits.hip, affix.hip, context.hip, files.hip, combine.hip): the classify kernel of a lane-local
// predicate, the scatter kernel, and the launcher.  A pass is a struct of its own parameters, passed to the kernels by value:
//
//   bool Selected(uint64_t i) const              string i is selected (i < n); only where the predicate is one lane's own
//   void Write(uint64_t rank, uint64_t i) const  what the selected string i, the rank-th of them, leaves (rank < cap)
//
// A pass whose classify is a matter of the whole block (an LDS table, tile sums, a slice of a list) keeps a classify kernel
// of its own that ends in TileBallot, and launches it between Front() and Scan().  The templates are instantiated in the
// pass's unit only; the pass's struct carries its name, and so do its kernels' symbols.
#pragma once

#include "compact.h"
#include "internal.h"

namespace pirehip {

template <class Pass>
__global__ __launch_bounds__(kBlockThreads) void TileClassifyKernel(Pass p, uint64_t n, TileScratch s)
{
	__shared__ uint32_t waveCount[kBlockWaves];
	for (uint32_t tile = blockIdx.x; tile < s.tiles; tile += gridDim.x) {
		const uint64_t i = uint64_t(tile) * kBlockThreads + threadIdx.x;
		TileBallot(i < n && p.Selected(i), tile, s.ballots, s.tileCounts, waveCount);
	}
}

template <class Pass>
__global__ __launch_bounds__(kBlockThreads) void TileScatterKernel(Pass p, TileScratch s, uint64_t cap)
{
	for (uint32_t tile = blockIdx.x; tile < s.tiles; tile += gridDim.x) {
		bool selected;
		const uint64_t rank = TileRank(tile, s.ballots, s.tileCounts, &selected);
		if (selected && rank < cap)   // (a selected bit: i < n)
			p.Write(rank, uint64_t(tile) * kBlockThreads + threadIdx.x);
	}
}

// The launcher of one compaction on `stream`, in the order of its launches: Front(), the classify -- Classify() or the
// pass's own kernel on Grid() --, Scan(), Scatter(), Done(); Tail() is the last three.  What a pass enqueues of its own
// stands between these calls where it stood before.  Declared in front of the pass's further scratch: freed behind it.
struct TilePass {
	const hipStream_t stream;
	StreamScratch scratch;
	TileScratch s = {};
	explicit TilePass(hipStream_t stream_) : stream(stream_), scratch(stream_) {}
	// n == 0: *outCount is zeroed on the stream and s.tiles stays 0 (nothing to launch); 2^32 strings or more: refused in `who`'s name
	int Front(const char* who, const char* scratchLabel, uint64_t n, uint64_t* outCount)
	{
		return TileCompaction(who, scratchLabel, n, outCount, stream, scratch, &s);
	}
	dim3 Grid() const { return dim3(std::min(s.tiles, kTileMaxBlocks)); }
	template <class Pass>
	void Classify(const Pass& p, uint64_t n) const
	{
		hipLaunchKernelGGL(TileClassifyKernel<Pass>, Grid(), dim3(kBlockThreads), 0, stream, p, n, s);
	}
	void Scan(uint64_t* outCount) const { LaunchTileScan(s.tileCounts, 1, s.tiles, outCount, stream); }
	template <class Pass>
	void Scatter(const Pass& p, uint64_t cap) const
	{
		if (cap)
			hipLaunchKernelGGL(TileScatterKernel<Pass>, Grid(), dim3(kBlockThreads), 0, stream, p, s, cap);
	}
	int Done(const char* launchLabel) const
	{
		const hipError_t e = hipGetLastError();
		return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, launchLabel);
	}
	template <class Pass>
	int Tail(const Pass& p, uint64_t cap, uint64_t* outCount, const char* launchLabel) const
	{
		Scan(outCount);
		Scatter(p, cap);
		return Done(launchLabel);
	}
};

}  // namespace pirehip
