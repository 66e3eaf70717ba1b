// One column of every string on the device (pire_hip_fields): where field k of every string is.
//
// The text this library scans is records -- access logs, TSV exports --, and the question a caller has there is "which
// lines match in column 3".  This unit finds the column where the scan is; pire_hip_gather_spans turns what it writes into
// the batch that the scan takes.  String i is text[offsets[i], offsets[i + 1]); it holds m separator bytes at
// q_1 < ... < q_m (absolute in text), q_0 = offsets[i] - 1, q_{m+1} = offsets[i + 1]:
//
//   k <= m:   spans[2i] = q_k + 1      spans[2i + 1] = q_{k+1}      (REST: spans[2i + 1] = offsets[i + 1], `cut -f k-`)
//   k >  m:   spans[2i] = spans[2i + 1] = offsets[i + 1]
//
// The work is divided by BYTES: text[offsets[0], offsets[n]) is cut into tiles of 16 KiB on the 16-byte grid of its address,
// a lane loads 16 bytes (compact.h LoadLane, split.hip's load), and every block takes a run of consecutive tiles.  How many
// bytes there are only the device knows in a device-pointer call -- offsets[n] is read there, never back --, so the grid is
// fixed by the host and the kernels cut the tiles into as many runs as there are blocks; a block without tiles leaves.
//
//   defaults  one lane per string: spans[2i] = (k == 0 ? offsets[i] : offsets[i + 1]), spans[2i + 1] = offsets[i + 1] --
//             what holds for a string without a separator of rank k - 1 or k: every empty string, every short one.
//   count     per tile: the separators, and those behind the last string start inside the tile (one wave finds that start:
//             compact.h WaveOwner on the tile's last byte; both counts in one BlockExclusive).  A block folds its tiles into
//             ONE record: whether a string starts in its run, and the separators behind the last such start (or all).
//   carry     one block, a segmented sum over the records (1 024 a step, a 64-bit carry between the steps): the separators
//             of the string that is open at the first byte of every block's run, from the bytes in front of the run.
//   resolve   every block walks its run again with that carry.  Two waves find the strings that own the tile's first and
//             last byte; the boundaries between them are staged in LDS (a tile of more than 2 048 strings reads them from
//             memory); the lanes' exclusive separator counts and masks go to LDS too.  A lane WITH a separator finds the string
//             of its first one by binary search in the boundaries, and again from there for a separator that lies in a later
//             string (empty strings between two separators of a lane cost the logarithm of their number); the rank of a separator inside
//             its string = the count in front of it in the tile - the count in front of the string's start (LDS), or + the
//             carry for the string that was open when the tile began.  Rank k - 1 writes spans[2i] = p + 1, rank k writes
//             spans[2i + 1] = p: one writer per entry, the defaults pass is a launch earlier on the same stream.
//
// Four launches on the caller's stream, the shape of split.hip: the text is read twice, no block waits for another block,
// no atomics (the output is the same bits every time), scratch = 16 bytes per block of the grid (<= 2 048) from the
// stream-ordered allocator, whatever the text holds.  Plain HIP with compiler-placed waits: nothing here keeps data on its
// way in registers.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "compact.h"
#include "internal.h"

namespace pirehip {

namespace {

constexpr uint32_t kFldThreads = kBlockThreads;
constexpr uint32_t kFldWaves = kBlockWaves;
constexpr uint32_t kFldTile = PIRE_HIP_FIELDS_TILE_BYTES;   // 16 bytes a lane
constexpr uint32_t kFldMaxBlocks = 2048;                    // 2 blocks on each of 256 CUs, four rounds
constexpr uint32_t kFldStage = 2048;                        // string boundaries of a tile kept in LDS
static_assert(kFldTile == kFldThreads * 16, "one dwordx4 per lane and tile");

// What a block's run of tiles says to the runs behind it, one word: bit 63 = a string starts inside the run; bits 0..62 = the
// separators behind the last such start (all separators of the run if there is none)
constexpr uint64_t kFldStartBit = 1ull << 63;

struct FieldsParams {
	const uint8_t* text;
	const uint64_t* offsets;
	uint64_t n;
	uint32_t sep4;    // the separator in every byte
	uint32_t field;
	uint32_t rest;
	uint64_t* spans;
	uint64_t* records;       // [blocks]
	uint64_t* carry;         // [blocks] separators of the string open at the run's first byte, in front of the run
};

// The bytes text[offsets[0], offsets[n]) on the 16-byte grid of their address, and the tiles of this block
struct FieldsGeometry {
	const uint8_t* raw;
	uint64_t lo, size;
	uint32_t head;
	uint64_t tile0, tile1;   // the block's run [tile0, tile1)
	__device__ __forceinline__ FieldsGeometry(const FieldsParams& p)
	{
		lo = p.offsets[0];
		size = p.offsets[p.n] - lo;
		raw = p.text + lo;
		head = size ? uint32_t(reinterpret_cast<uintptr_t>(raw) & 15) : 0;
		const uint64_t tiles = (head + size + kFldTile - 1) / kFldTile;
		const uint64_t run = (tiles + gridDim.x - 1) / gridDim.x;
		tile0 = std::min(tiles, blockIdx.x * run);
		tile1 = std::min(tiles, tile0 + run);
	}
	// positions in text (absolute) of the tile's first byte and of the byte behind its last: lo <= first < last <= lo + size
	__device__ __forceinline__ uint64_t First(uint64_t tile) const { return lo + std::max<uint64_t>(tile * kFldTile, head) - head; }
	__device__ __forceinline__ uint64_t Last(uint64_t tile) const { return lo + std::min<uint64_t>((tile + 1) * kFldTile, head + size) - head; }
};

__global__ void FieldsDefaultsKernel(FieldsParams p)
{
	const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i < p.n) {
		const uint64_t end = p.offsets[i + 1];
		p.spans[2 * i] = p.field == 0 ? p.offsets[i] : end;
		p.spans[2 * i + 1] = end;
	}
}

__global__ __launch_bounds__(kFldThreads) void FieldsCountKernel(FieldsParams p)
{
	__shared__ uint32_t waveSum[kFldWaves];
	__shared__ uint64_t lastStart;
	const FieldsGeometry g(p);
	uint64_t since = 0;
	for (uint64_t tile = g.tile0; tile < g.tile1; ++tile) {
		const uint64_t v = tile * kFldTile + threadIdx.x * 16;
		uint32_t w[4], valid, total;
		const uint32_t dm = LoadLane(g.raw, g.head, g.size, p.sep4, v, w, &valid);
		if (threadIdx.x < 64) {
			const uint64_t owner = WaveOwner(p.offsets, p.n, g.Last(tile) - 1);
			if (threadIdx.x == 0)
				lastStart = p.offsets[owner];
		}
		__syncthreads();
		const uint64_t start = lastStart;   // (in front of the tile: no string starts inside it)
		// the lane's separators at or behind `start`: start's virtual position against the lane's
		const uint64_t sv = start - g.lo + g.head;
		const uint32_t behind = sv <= v ? dm : sv >= v + 16 ? 0 : dm & ~((1u << uint32_t(sv - v)) - 1);
		// both counts in one sum: 16 384 at most each
		(void)BlockExclusive(uint32_t(__popc(dm)) | uint32_t(__popc(behind)) << 16, waveSum, &total);
		const uint32_t all = total & 0xFFFFu, tail = total >> 16;
		if (start >= g.First(tile))
			since = kFldStartBit | tail;
		else
			since += all;
	}
	if (threadIdx.x == 0)
		p.records[blockIdx.x] = since;
}

// The segmented sum's operator: what the run b says behind what the runs in front of it said
__device__ __forceinline__ uint64_t FieldsCombine(uint64_t front, uint64_t b)
{
	return b & kFldStartBit ? b : front + b;   // (front's own start bit stays: the sum is below 2^63)
}

// carry[b] = the separators of the string that is open at the first byte of run b, counted over the runs in front of it
__global__ __launch_bounds__(kFldThreads) void FieldsCarryKernel(FieldsParams p, uint32_t blocks)
{
	__shared__ uint64_t waveLast[kFldWaves];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint64_t carry = 0;   // the inclusive value of the last run of the step before
	for (uint32_t base = 0; base < blocks; base += kFldThreads) {
		const uint32_t b = base + threadIdx.x;
		uint64_t incl = b < blocks ? p.records[b] : 0;
		for (uint32_t d = 1; d < 64; d <<= 1) {
			const uint64_t up = ShuffleUp(incl, d);
			if (lane >= d)
				incl = FieldsCombine(up, incl);
		}
		if (lane == 63)
			waveLast[wave] = incl;
		__syncthreads();
		uint64_t front = carry & ~kFldStartBit, all = front;
		for (uint32_t w = 0; w < kFldWaves; ++w) {
			all = FieldsCombine(all, waveLast[w]) & ~kFldStartBit;
			if (w + 1 == wave)
				front = all;
		}
		__syncthreads();   // (the next step writes waveLast again)
		const uint64_t mine = FieldsCombine(front, incl) & ~kFldStartBit;
		// exclusive: the run behind this one starts with what this one ends with
		if (b + 1 < blocks)
			p.carry[b + 1] = mine;
		carry = all;
	}
	if (threadIdx.x == 0)
		p.carry[0] = 0;
}

// An entry of offsets as the lanes of a tile want it: relative to the tile's first byte, cut to [0, tile + 16]
__device__ __forceinline__ uint32_t FieldsRelBound(uint64_t off, uint64_t first)
{
	return off <= first ? 0 : uint32_t(std::min<uint64_t>(off - first, kFldTile + 16));
}

__global__ __launch_bounds__(kFldThreads) void FieldsResolveKernel(FieldsParams p)
{
	__shared__ uint32_t waveSum[kFldWaves];
	__shared__ uint32_t laneFront[kFldThreads];   // separators of the tile in front of the lane's bytes
	__shared__ uint16_t laneMask[kFldThreads];    // the lane's separators
	__shared__ uint32_t bound[kFldStage + 1];     // where the tile's strings begin (FieldsRelBound)
	__shared__ uint64_t owner[2];
	const FieldsGeometry g(p);
	uint64_t carry = g.tile0 < g.tile1 ? p.carry[blockIdx.x] : 0;
	for (uint64_t tile = g.tile0; tile < g.tile1; ++tile) {
		const uint64_t first = g.First(tile), last = g.Last(tile);
		const uint64_t v = tile * kFldTile + threadIdx.x * 16;
		uint32_t w[4], valid, total;
		const uint32_t dm = LoadLane(g.raw, g.head, g.size, p.sep4, v, w, &valid);
		const uint32_t wave = threadIdx.x >> 6;
		if (wave < 2) {
			const uint64_t o = WaveOwner(p.offsets, p.n, wave == 0 ? first : last - 1);
			if ((threadIdx.x & 63) == 0)
				owner[wave] = o;
		}
		const uint32_t front = BlockExclusive(uint32_t(__popc(dm)), waveSum, &total);   // (its barriers publish owner[] too)
		laneFront[threadIdx.x] = front;
		laneMask[threadIdx.x] = uint16_t(dm);
		const uint64_t s0 = owner[0];
		const uint64_t count = owner[1] - s0 + 1;   // the strings with bytes in the tile: s0 .. s0 + m - 1
		const bool staged = count <= kFldStage;
		const uint32_t m = uint32_t(count);         // (n < 2^32)
		if (staged)
			for (uint32_t i = threadIdx.x; i <= m; i += kFldThreads)
				bound[i] = FieldsRelBound(p.offsets[s0 + i], first);
		__syncthreads();
		// Bound(0) = 0 <= every position of the tile < Bound(m)
		auto Bound = [&](uint32_t i) { return staged ? bound[i] : FieldsRelBound(p.offsets[s0 + i], first); };
		// separators of the tile in front of relative position x (< the tile's length)
		const uint32_t shift = uint32_t(first - g.lo + g.head - tile * kFldTile);   // the first tile of a misaligned text begins inside its first lane
		auto Front = [&](uint32_t x) {
			const uint32_t at = x + shift;
			return laneFront[at >> 4] + uint32_t(__popc(uint32_t(laneMask[at >> 4]) & ((1u << (at & 15)) - 1)));
		};
		const bool openBefore = p.offsets[s0] < first;   // string s0 began in front of the tile: the carry is its
		if (dm) {
			uint32_t j = 0, next = 0;   // (next = 0: the first separator searches)
			uint64_t base = 0;   // what to take off a separator's count in the tile to get its rank in string s0 + j
			for (uint32_t mm = dm; mm; mm &= mm - 1) {
				const uint32_t bit = uint32_t(__ffs(int(mm))) - 1;
				const uint64_t pos = g.lo + (v + bit - g.head);            // absolute in text
				const uint32_t rel = uint32_t(pos - first);
				// the separator lies in a later string than the lane's last one (or is its first): the last j with Bound(j) <= rel,
				// by binary search from where the lane is -- any number of empty strings in between costs log2 of it
				if (next <= rel) {
					uint32_t end = m;   // Bound(j) <= rel < Bound(m): Bound(m) is behind the tile's last byte
					while (end - j > 1) {
						const uint32_t mid = (j + end) / 2;
						if (Bound(mid) <= rel)
							j = mid;
						else
							end = mid;
					}
					next = Bound(j + 1);
					base = j == 0 ? (openBefore ? 0 - carry : 0) : uint64_t(Front(Bound(j)));
				}
				const uint64_t rank = uint64_t(front + uint32_t(__popc(dm & ((1u << bit) - 1)))) - base;
				const uint64_t i = s0 + j;
				if (rank + 1 == p.field)
					p.spans[2 * i] = pos + 1;
				if (rank == p.field && !p.rest)
					p.spans[2 * i + 1] = pos;
			}
		}
		// what the next tile of the run starts with: the separators behind the last start inside this tile, or all on top
		const uint64_t lastBegin = p.offsets[owner[1]];
		if (lastBegin >= first)
			carry = total - Front(uint32_t(lastBegin - first));
		else
			carry += total;
		__syncthreads();   // (the next tile writes owner and the LDS arrays again)
	}
}

}  // namespace

int LaunchFields(const void* text, const uint64_t* offsets, uint64_t n, uint32_t sep, uint32_t field, uint32_t mode, uint64_t* outSpans,
                 uint64_t bytesHint, hipStream_t stream)
{
	if (n == 0)
		return PIRE_HIP_OK;
	if (n >= (1ull << 32)) {
		SetError("pire_hip_fields: 2^32 strings or more in one call");
		return PIRE_HIP_EUNSUPPORTED;
	}
	// as many blocks as the text has tiles where the host knows its size (a misaligned text: one tile more), else all of them
	const uint32_t blocks = uint32_t(std::min<uint64_t>(bytesHint == kFieldsBytesUnknown ? kFldMaxBlocks : bytesHint / kFldTile + 2, kFldMaxBlocks));
	StreamScratch scratch(stream);
	if (int rc = scratch.Alloc(size_t(blocks) * 16, "hipMallocAsync(fields scratch)"))
		return rc;
	FieldsParams p;
	p.text = static_cast<const uint8_t*>(text);
	p.offsets = offsets;
	p.n = n;
	p.sep4 = (sep & 0xFFu) * 0x01010101u;
	p.field = field;
	p.rest = mode & PIRE_HIP_FIELDS_REST;
	p.spans = outSpans;
	p.records = scratch.as<uint64_t>();
	p.carry = p.records + blocks;
	hipLaunchKernelGGL(FieldsDefaultsKernel, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, stream, p);
	hipLaunchKernelGGL(FieldsCountKernel, dim3(blocks), dim3(kFldThreads), 0, stream, p);
	hipLaunchKernelGGL(FieldsCarryKernel, dim3(1), dim3(kFldThreads), 0, stream, p, blocks);
	hipLaunchKernelGGL(FieldsResolveKernel, dim3(blocks), dim3(kFldThreads), 0, stream, p);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "fields launch");
}

}  // namespace pirehip
