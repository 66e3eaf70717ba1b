// The pieces the hit passes share on the device (the eight ballot compactions, route.hip, split.hip, gather.hip,
// fields.hip): the prefix sum over a block of 1 024 threads, the ballot compaction of a tile of 1 024 strings, the 16-byte
// lane load of the byte-rate passes, the wave-wide searches in an offsets array and in a hit list, and the load of a list
// entry of any alignment.  Device only, force-inlined into the kernels that use them; tile_pass.h builds the kernel pair and
// the launcher of the ballot compactions on them; DESIGN.md section 4.15 says who owns what.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace pirehip {

constexpr uint32_t kBlockThreads = 1024;   // every kernel that uses these pieces is launched with this many threads ...
constexpr uint32_t kBlockWaves = kBlockThreads / 64;   // ... one tile of the compaction = 1 024 strings = 16 ballot words
constexpr uint32_t kTileMaxBlocks = 8192;  // the grid of a kernel that walks tiles: no larger, tiles in a grid-stride loop

// The scratch of one ballot compaction (select.hip TileCompaction carves it out of one allocation)
struct TileScratch {
	uint64_t* ballots;      // [tiles * 16] selected bits, one word per wave
	uint32_t* tileCounts;   // [tiles] selected strings per tile; after the scan: selected strings in front of the tile
	uint32_t tiles;
};

__device__ __forceinline__ uint32_t ShuffleUp(uint32_t v, uint32_t d) { return uint32_t(__shfl_up(int(v), int(d), 64)); }
__device__ __forceinline__ uint64_t ShuffleUp(uint64_t v, uint32_t d) { return __shfl_up(static_cast<unsigned long long>(v), d, 64); }

// The sum of v over the lanes in front of this one in the block, and over all of them (waveSum: 16 words of LDS).  Two
// barriers: the call may be repeated at once.
template <class T>
__device__ __forceinline__ T BlockExclusive(T v, T* waveSum, T* total)
{
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	T incl = v;
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const T up = ShuffleUp(incl, d);
		if (lane >= d)
			incl += up;
	}
	if (lane == 63)
		waveSum[wave] = incl;
	__syncthreads();
	T before = 0, all = 0;
	for (uint32_t w = 0; w < kBlockWaves; ++w) {
		const T ws = waveSum[w];
		before += w < wave ? ws : 0;
		all += ws;
	}
	__syncthreads();   // (the next call writes waveSum again)
	*total = all;
	return before + incl - v;
}

// The classify tail of a ballot compaction: the selected bits of the wave are one ballot word, kept in
// ballots[tile * 16 + wave]; tileCounts[tile] = the selected strings of the tile (waveCount: 16 words of LDS).
__device__ __forceinline__ void TileBallot(bool sel, uint32_t tile, uint64_t* ballots, uint32_t* tileCounts, uint32_t* waveCount)
{
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t ballot = __ballot(sel);
	if (lane == 0) {
		ballots[size_t(tile) * kBlockWaves + wave] = ballot;
		waveCount[wave] = uint32_t(__popcll(ballot));
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t sum = 0;
		for (uint32_t w = 0; w < kBlockWaves; ++w)
			sum += waveCount[w];
		tileCounts[tile] = sum;
	}
	__syncthreads();
}

// The scatter head: *selected = this lane's string was selected; its rank among the selected strings of the batch = the
// scanned tile count + the popcounts of the waves in front + mbcnt of its own wave's ballot word: ascending, no atomics.
__device__ __forceinline__ uint64_t TileRank(uint32_t tile, const uint64_t* ballots, const uint32_t* tileCounts, bool* selected)
{
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t* words = ballots + size_t(tile) * kBlockWaves;
	// lanes 0..15 hold the tile's ballot words: the selected strings of the waves in front of this one ...
	const uint64_t word = lane < kBlockWaves ? words[lane] : 0;
	uint32_t front = lane < wave ? uint32_t(__popcll(word)) : 0;
	for (uint32_t d = 1; d < 64; d <<= 1)
		front += uint32_t(__shfl_xor(int(front), int(d), 64));   // (over all 64 lanes: every lane ends with the sum)
	// ... and this wave's own word
	const uint32_t lo = uint32_t(__shfl(int(uint32_t(word)), int(wave), 64));
	const uint32_t hi = uint32_t(__shfl(int(uint32_t(word >> 32)), int(wave), 64));
	const uint64_t mine = (uint64_t(hi) << 32) | lo;
	*selected = (mine >> lane) & 1;
	return uint64_t(tileCounts[tile]) + front + __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0));
}

// The lane's 16 bytes of the byte-rate passes (split.hip, fields.hip) at virtual position v (a multiple of 16; raw[0] is at
// virtual position head = raw's address modulo 16, the buffer is `size` bytes): w = the bytes (0 where the buffer is not),
// *valid = which of them are the buffer's; returns which of those are the byte that byte4 holds four times.  A lane inside
// the buffer loads with one global_load_dwordx4, the lanes that hang over its two ends load their bytes one by one.
__device__ __forceinline__ uint32_t LoadLane(const uint8_t* raw, uint32_t head, uint64_t size, uint32_t byte4, uint64_t v, uint32_t (&w)[4],
                                             uint32_t* valid)
{
	const uint64_t end = head + size;
	if (v >= head && v + 16 <= end) {
		const uint4 q = *reinterpret_cast<const uint4*>(raw + ptrdiff_t(v - head));
		w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
		*valid = 0xFFFFu;
	} else {
		uint32_t vm = 0;
		w[0] = w[1] = w[2] = w[3] = 0;
		const uint8_t* b = raw + ptrdiff_t(v - head);   // (in front of raw for the first lane of a misaligned buffer: not read there)
#pragma unroll
		for (uint32_t i = 0; i < 16; ++i)
			if (v + i >= head && v + i < end) {
				w[i >> 2] |= uint32_t(b[i]) << (8 * (i & 3));
				vm |= 1u << i;
			}
		*valid = vm;
	}
	uint32_t dm = 0;
#pragma unroll
	for (uint32_t k = 0; k < 4; ++k) {
		const uint32_t x = w[k] ^ byte4;
		const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 in every byte of x that is 0, exactly
		dm |= (((t >> 7) | (t >> 14) | (t >> 21) | (t >> 28)) & 0xFu) << (4 * k);
	}
	return dm & *valid;
}

// The string that owns byte pos of a batch -- the last j < k with off[j] <= pos; off[0] <= pos < off[k] --, found by one
// wave: 64 probes a step.  It steps over the repeated entries that empty strings leave.
__device__ __forceinline__ uint64_t WaveOwner(const uint64_t* off, uint64_t k, uint64_t pos)
{
	const uint32_t lane = threadIdx.x & 63;
	uint64_t lo = 0, hi = k;
	while (hi - lo > 1) {
		const uint64_t step = (hi - lo + 63) / 64;
		const uint64_t q = lo + (lane + 1) * step;
		const bool le = q < hi && off[q] <= pos;   // true in the first c lanes, false behind them
		const uint64_t c = uint64_t(__popcll(__ballot(le)));
		hi = std::min(hi, lo + (c + 1) * step);
		lo += c * step;
	}
	return lo;
}

// Entry j of a hit list: `list` may have any alignment, the entry is read through a packed type
struct __attribute__((packed, aligned(1))) UnalignedU64 {
	uint64_t v;
};

__device__ __forceinline__ uint64_t LoadU64(const uint64_t* list, uint64_t j)
{
	return reinterpret_cast<const UnalignedU64*>(list)[j].v;
}

// How many of a[0, m) are < x -- kInclusive: <= x -- (the array does not decrease; any alignment), found by one wave: 64
// probes a step, every probe inside [0, m)
template <bool kInclusive>
__device__ __forceinline__ uint64_t WaveBound(const uint64_t* a, uint64_t m, uint64_t x)
{
	const uint32_t lane = threadIdx.x & 63;
	uint64_t lo = 0, hi = m;   // the answer is in [lo, hi]
	while (hi > lo) {
		const uint64_t step = (hi - lo + 63) / 64;
		const uint64_t q = lo + (lane + 1) * step - 1;
		const bool in = q < hi && (kInclusive ? LoadU64(a, q) <= x : LoadU64(a, q) < x);   // true in the first c lanes, false behind them
		const uint64_t c = uint64_t(__popcll(__ballot(in)));
		hi = std::min(hi, lo + (c + 1) * step - 1);
		lo = std::min(lo + c * step, hi);   // (the min: an array that decreases)
	}
	return lo;
}

}  // namespace pirehip
