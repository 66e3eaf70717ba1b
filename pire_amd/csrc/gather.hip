// The listed strings of a batch, back to back (pire_hip_gather): from a hit list to bytes without leaving the device.
//
// Every scan entry point takes text + offsets[n + 1]; what pire_hip_select and pire_hip_run_lines_select hand back is a
// list of indices or of [begin, end) ranges.  This unit turns such a list into text' + offsets' again -- the input of the
// next scan (a second scanner on the survivors of a first one) or, with a tail byte behind every string, grep's output:
//
//   k = min(*count, cap)     L_j = length of source string j + a (a = 1 with a tail byte)
//   outOffsets[0] = 0        outOffsets[j + 1] = L_0 + ... + L_j        *outBytes = outOffsets[k]
//
//   lengths   one lane per output string: L_j, with the bounds check of its index or span (out of range: an empty string);
//             one 64-bit sum per tile of 1 024 strings.  The sum of tile t waits in outOffsets[1024 t + 1], an entry the
//             tile's own first string owns and the offsets pass overwrites: the pass needs NO SCRATCH, so a call makes no
//             allocation of any kind (an allocation behind a free that is still pending on a busy stream is where the
//             runtime made the second of two enqueue-only calls wait).
//   scan      exclusive scan of the tile sums, one block, a 64-bit carry between its steps; the total is *outBytes.
//   offsets   every tile reads its base, computes its lengths again: outOffsets[j + 1] = tile base + the inclusive scan
//             inside the tile.
//   copy      the work is divided by OUTPUT BYTES.  outText is cut into tiles of 16 KiB on the 16-byte grid of its address;
//             a block finds the strings that own its tile's first and last byte by search in outOffsets (64 probes a step,
//             one wave each, compact.h WaveOwner; the owner of byte x is the LAST j with outOffsets[j] <= x, which steps over the repeated
//             entries that empty strings leave), stages the tile's string boundaries and source positions in LDS -- one
//             entry per lane and store, consecutive lanes at consecutive words --, and then every lane owns 16 output
//             bytes: it finds its string by binary search in the staged boundaries; if its 16 bytes lie inside one string
//             it fetches them with one unaligned 16-byte load; otherwise (a boundary, a tail byte, the partial groups at
//             the two ends of outText) it goes PIECE BY PIECE: for every string that has bytes in the group, the one or two
//             aligned 16-byte chunks of the source that hold them (chunks that hold at least one byte of the string:
//             inside its page), realigned with v_alignbyte_b32 and merged under a byte mask; the tail bytes are set in
//             between.  Whole groups leave as one global_store_dwordx4, the partial ones at outText's two ends by bytes.  A string of
//             3 MiB spreads over about 190 blocks, 300 empty strings cost nothing.  A tile of more strings than the stage
//             holds (2 048: strings of under 8 bytes on average) reads boundaries and sources from global memory instead.
//
// The block-wide prefix sum of the first three kernels is compact.h's BlockExclusive, over 64-bit sums.
// Four launches on the caller's stream, the shape of select.hip and split.hip: no block waits for another block, no
// atomics (the output is the same bits every time), no scratch.  Plain HIP with compiler-placed waits: nothing here keeps data on its way in registers.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "compact.h"
#include "internal.h"

namespace pirehip {

namespace {

constexpr uint32_t kGatThreads = kBlockThreads;
constexpr uint32_t kGatWaves = kBlockWaves;
constexpr uint32_t kGatTile = PIRE_HIP_GATHER_TILE_BYTES;   // 16 output bytes a lane
constexpr uint32_t kGatStage = 2048;                        // string boundaries of a tile kept in LDS: 4 + 8 bytes each
constexpr uint32_t kGatMaxBlocks = 2048;                    // 2 blocks on each of 256 CUs, four rounds; tiles in a grid-stride loop
static_assert(kGatTile == kGatThreads * 16, "one dwordx4 per lane and tile");

struct GatherParams {
	GatherSource src;
	const uint64_t* count;   // nullable: cap strings
	uint64_t cap;
	uint32_t a;              // 1: a tail byte behind every string
	uint32_t tailByte;
	uint8_t* outText;
	uint64_t textCap;
	uint64_t* outOffsets;
	uint64_t* outBytes;
};

// Where the byte count of tile t of the strings waits between the passes (after the scan: the bytes in front of the tile):
// the outOffsets entry of the tile's first string, which exists because the tile has one, and which the offsets pass writes last
__device__ __forceinline__ uint64_t* TileSum(const GatherParams& p, uint64_t tile)
{
	return p.outOffsets + (tile * kGatThreads + 1);
}

__device__ __forceinline__ uint64_t Strings(const GatherParams& p)
{
	return p.count && p.cap ? std::min(*p.count, p.cap) : p.cap;
}

// Where output string j comes from: text[*begin, *begin + *len).  An index or a span out of range is an empty string
// whose position is never read.
__device__ __forceinline__ void Range(const GatherSource& s, uint64_t j, uint64_t* begin, uint64_t* len)
{
	uint64_t b = 0, e = 0;
	if (s.spans) {
		b = s.spans[2 * j], e = s.spans[2 * j + 1];
		if (e > s.size)
			e = 0;
	} else {
		const uint64_t i = s.idx ? s.idx[j] : j;
		if (i < s.n)
			b = s.offsets[i], e = s.offsets[i + 1];
	}
	const bool ok = b <= e;
	*begin = ok ? b : 0;
	*len = ok ? e - b : 0;
}

__device__ __forceinline__ uint64_t Length(const GatherParams& p, uint64_t j, uint64_t k)
{
	if (j >= k)
		return 0;
	uint64_t begin, len;
	Range(p.src, j, &begin, &len);
	return len + p.a;
}

__global__ __launch_bounds__(kGatThreads) void GatherLengthsKernel(GatherParams p)
{
	__shared__ uint64_t waveSum[kGatWaves];
	const uint64_t k = Strings(p);
	for (uint64_t base = uint64_t(blockIdx.x) * kGatThreads; base < k; base += uint64_t(gridDim.x) * kGatThreads) {
		uint64_t total;
		(void)BlockExclusive(Length(p, base + threadIdx.x, k), waveSum, &total);
		if (threadIdx.x == 0)
			*TileSum(p, base / kGatThreads) = total;
	}
}

// *TileSum(t) = bytes in front of tile t, *outBytes = the total; the entry no string stands for: outOffsets[0]
__global__ __launch_bounds__(kGatThreads) void GatherScanKernel(GatherParams p)
{
	__shared__ uint64_t waveSum[kGatWaves];
	const uint64_t k = Strings(p);
	const uint64_t tiles = (k + kGatThreads - 1) / kGatThreads;
	uint64_t carry = 0;
	for (uint64_t base = 0; base < tiles; base += kGatThreads) {
		const uint64_t i = base + threadIdx.x;
		const uint64_t v = i < tiles ? *TileSum(p, i) : 0;
		uint64_t total;
		const uint64_t front = BlockExclusive(v, waveSum, &total);
		if (i < tiles)
			*TileSum(p, i) = carry + front;
		carry += total;
	}
	if (threadIdx.x == 0) {
		*p.outBytes = carry;
		if (p.outOffsets)
			p.outOffsets[0] = 0;
	}
}

__global__ __launch_bounds__(kGatThreads) void GatherOffsetsKernel(GatherParams p)
{
	__shared__ uint64_t waveSum[kGatWaves];
	const uint64_t k = Strings(p);
	for (uint64_t base = uint64_t(blockIdx.x) * kGatThreads; base < k; base += uint64_t(gridDim.x) * kGatThreads) {
		const uint64_t j = base + threadIdx.x;
		const uint64_t front = *TileSum(p, base / kGatThreads);   // (read by every lane before the barriers of the scan, written behind them)
		uint64_t total;
		const uint64_t len = Length(p, j, k);
		const uint64_t incl = BlockExclusive(len, waveSum, &total) + len;   // (inclusive: the entry BEHIND string j)
		if (j < k)
			p.outOffsets[j + 1] = front + incl;
	}
}

// An entry of outOffsets as the lanes of a tile want it: relative to the tile's first byte, cut to [0, tile + 16]
__device__ __forceinline__ uint32_t RelBound(uint64_t off, uint64_t tileLo)
{
	return off <= tileLo ? 0 : uint32_t(std::min<uint64_t>(off - tileLo, kGatTile + 16));
}

// The tile's strings s0 .. s0 + m - 1 as a lane reads them: Bound(i) = where string s0 + i begins (RelBound), Delta(i) =
// what to add to an output position inside it to get the position in the source text.
struct StagedStrings {
	const uint32_t* bound;
	const uint64_t* delta;
	__device__ __forceinline__ uint32_t Bound(uint32_t i) const { return bound[i]; }
	__device__ __forceinline__ uint64_t Delta(uint32_t i) const { return delta[i]; }
};
struct DirectStrings {
	const GatherParams& p;
	uint64_t s0, tileLo;
	__device__ __forceinline__ uint32_t Bound(uint32_t i) const { return RelBound(p.outOffsets[s0 + i], tileLo); }
	__device__ __forceinline__ uint64_t Delta(uint32_t i) const
	{
		uint64_t begin, len;
		Range(p.src, s0 + i, &begin, &len);
		return begin - p.outOffsets[s0 + i];
	}
};

struct __attribute__((packed, aligned(1))) Unaligned16 {
	uint32_t w[4];
};

// The whole-group lanes' load: one unaligned global_load_dwordx4 (the product), or the two aligned chunks of the pieces'
// path (a timing-experiment build, `make exp N=1`: DESIGN.md section 4.12 has both)
#if defined(PIRE_EXP) && PIRE_EXP == 1
constexpr bool kGatUnalignedLoad = false;
#else
constexpr bool kGatUnalignedLoad = true;
#endif

// 0xFF in bytes [from, to) of dword k of a 16-byte group, 0 <= from <= to <= 16
__device__ __forceinline__ uint32_t ByteMask(uint32_t k, uint32_t from, uint32_t to)
{
	const uint32_t a = std::min(std::max(from, 4 * k), 4 * k + 4) - 4 * k, b = std::min(std::max(to, 4 * k), 4 * k + 4) - 4 * k;   // 0..4
	const uint32_t below = b == 4 ? 0xFFFFFFFFu : (1u << (8 * b)) - 1, under = a == 4 ? 0xFFFFFFFFu : (1u << (8 * a)) - 1;
	return below & ~under;
}

// Bytes [from, to) of the 16-byte window that begins at `window` (any alignment; it may begin in front of the string and
// end behind it) into w: the aligned chunks that hold one of THOSE bytes are loaded, no other.
__device__ __forceinline__ void MergePiece(const uint8_t* window, uint32_t from, uint32_t to, uint32_t (&w)[4])
{
	const uintptr_t ws = reinterpret_cast<uintptr_t>(window);
	const uintptr_t c0 = ws & ~uintptr_t(15);
	const uint32_t shift = uint32_t(ws & 15);
	uint4 q0 = make_uint4(0, 0, 0, 0), q1 = make_uint4(0, 0, 0, 0);
	if (c0 + 16 > ws + from)
		q0 = *reinterpret_cast<const uint4*>(c0);
	if (c0 + 16 < ws + to)
		q1 = *reinterpret_cast<const uint4*>(c0 + 16);
	// dwords shift / 4 .. shift / 4 + 4 of the two chunks (selects, no indexing: everything stays in registers)
	const bool one = shift & 4, two = shift & 8;
	const uint32_t t0 = one ? q0.y : q0.x, t1 = one ? q0.z : q0.y, t2 = one ? q0.w : q0.z, t3 = one ? q1.x : q0.w;
	const uint32_t t4 = one ? q1.y : q1.x, t5 = one ? q1.z : q1.y, t6 = one ? q1.w : q1.z;
	const uint32_t e[5] = {two ? t2 : t0, two ? t3 : t1, two ? t4 : t2, two ? t5 : t3, two ? t6 : t4};
#pragma unroll
	for (uint32_t k = 0; k < 4; ++k) {
		const uint32_t mask = ByteMask(k, from, to);
		w[k] = (w[k] & ~mask) | (__builtin_amdgcn_alignbyte(e[k + 1], e[k], shift & 3) & mask);
	}
}

// The lane's output bytes [lo, hi) -- a whole 16-byte group of outText's grid, or the part of one that lies inside
// [0, limit) -- out of the m strings of the tile.
template <class Strings>
__device__ __forceinline__ void CopyLane(const GatherParams& p, const Strings& s, uint32_t m, uint64_t tileLo, uint64_t lo, uint64_t hi)
{
	const uint32_t loRel = uint32_t(lo - tileLo), hiRel = uint32_t(hi - tileLo);
	uint32_t j = 0, end = m;   // the last j with Bound(j) <= loRel: Bound(0) = 0, Bound(m) > loRel
	while (end - j > 1) {
		const uint32_t mid = (j + end) / 2;
		if (s.Bound(mid) <= loRel)
			j = mid;
		else
			end = mid;
	}
	uint32_t next = s.Bound(j + 1);   // > loRel
	uint64_t delta = s.Delta(j);
	const uint8_t* text = p.src.text;
	uint32_t w[4] = {0, 0, 0, 0};
	if (kGatUnalignedLoad && hi - lo == 16 && next - p.a >= hiRel) {
		const Unaligned16 q = *reinterpret_cast<const Unaligned16*>(text + (lo + delta));
		w[0] = q.w[0], w[1] = q.w[1], w[2] = q.w[2], w[3] = q.w[3];
	} else {
		const uint32_t bytes = hiRel - loRel;   // 1..16; byte i of the lane is output position lo + i
		uint32_t i = 0;
		while (i < bytes) {
			while (next <= loRel + i) {   // (empty strings in between; Bound(m) is behind the tile's last byte)
				++j;
				next = s.Bound(j + 1);
				delta = s.Delta(j);
			}
			const uint32_t to = std::min(next - p.a, hiRel) - loRel;   // the string's own bytes end here (next >= 1)
			if (i < to) {
				MergePiece(text + (lo + delta), i, to, w);
				i = to;
			}
			if (p.a && i < bytes && loRel + i == next - 1) {
#pragma unroll
				for (uint32_t k = 0; k < 4; ++k)
					w[k] = (w[k] & ~ByteMask(k, i, i + 1)) | ((p.tailByte * 0x01010101u) & ByteMask(k, i, i + 1));
				++i;
			}
		}
	}
	uint8_t* dst = p.outText + lo;
	if (hi - lo == 16)
		*reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);   // 16-byte aligned: lo is on outText's grid
	else
#pragma unroll
		for (uint32_t i = 0; i < 16; ++i)   // (unrolled: w stays in registers)
			if (i < uint32_t(hi - lo))
				dst[i] = uint8_t(w[i >> 2] >> (8 * (i & 3)));
}

__global__ __launch_bounds__(kGatThreads) void GatherCopyKernel(GatherParams p)
{
	__shared__ uint32_t bound[kGatStage + 1];
	__shared__ uint64_t delta[kGatStage];
	__shared__ uint64_t owner[2];
	const uint64_t k = Strings(p);
	const uint64_t limit = std::min(*p.outBytes, p.textCap);   // output bytes [0, limit) are written
	// outText's address modulo 16: tiles and groups are counted from the 16-byte boundary in front of it
	const uint64_t head = reinterpret_cast<uintptr_t>(p.outText) & 15;
	const uint64_t tiles = limit ? (head + limit + kGatTile - 1) / kGatTile : 0;
	for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
		const uint64_t tileLo = std::max(tile * kGatTile, head) - head;              // output positions
		const uint64_t tileHi = std::min((tile + 1) * kGatTile, head + limit) - head;   // tileLo < tileHi <= limit <= outOffsets[k]
		const uint32_t wave = threadIdx.x >> 6;
		if (wave < 2) {
			const uint64_t o = WaveOwner(p.outOffsets, k, wave == 0 ? tileLo : tileHi - 1);
			if ((threadIdx.x & 63) == 0)
				owner[wave] = o;
		}
		__syncthreads();
		const uint64_t s0 = owner[0];
		const uint64_t count = owner[1] - s0 + 1;
		const bool staged = count <= kGatStage;
		const uint32_t m = uint32_t(count);   // (k < 2^32)
		if (staged) {
			for (uint32_t i = threadIdx.x; i <= m; i += kGatThreads) {
				const uint64_t off = p.outOffsets[s0 + i];
				bound[i] = RelBound(off, tileLo);
				if (i < m) {
					uint64_t begin, len;
					Range(p.src, s0 + i, &begin, &len);
					delta[i] = begin - off;
				}
			}
			__syncthreads();
		}
		const uint64_t v = tile * kGatTile + threadIdx.x * 16;   // the lane's group, on outText's grid
		const uint64_t lo = std::max(v, head) - head;
		const uint64_t hi = std::min(v + 16, head + limit) - head;   // (v + 16 > head: head < 16)
		if (lo < hi) {
			if (staged)
				CopyLane(p, StagedStrings{bound, delta}, m, tileLo, lo, hi);
			else
				CopyLane(p, DirectStrings{p, s0, tileLo}, m, tileLo, lo, hi);
		}
		__syncthreads();   // (the next tile writes owner and the stage again)
	}
}

}  // namespace

int LaunchGather(const GatherSource& src, const uint64_t* count, uint64_t cap, uint32_t tail, void* outText, uint64_t textCap,
                 uint64_t* outOffsets, uint64_t* outBytes, uint64_t hostTotal, hipStream_t stream)
{
	GatherParams p;
	p.src = src;
	p.count = count;
	p.cap = cap;
	p.a = tail != PIRE_HIP_GATHER_NO_TAIL ? 1 : 0;
	p.tailByte = tail & 0xFFu;
	p.outText = static_cast<uint8_t*>(outText);
	p.textCap = textCap;
	p.outOffsets = outOffsets;
	p.outBytes = outBytes;
	const uint64_t stringTiles = (cap + kGatThreads - 1) / kGatThreads;
	const dim3 stringGrid(uint32_t(std::min<uint64_t>(stringTiles, kGatMaxBlocks)));
	if (stringTiles)
		hipLaunchKernelGGL(GatherLengthsKernel, stringGrid, dim3(kGatThreads), 0, stream, p);
	hipLaunchKernelGGL(GatherScanKernel, dim3(1), dim3(kGatThreads), 0, stream, p);
	if (stringTiles)
		hipLaunchKernelGGL(GatherOffsetsKernel, stringGrid, dim3(kGatThreads), 0, stream, p);
	// the copy pass: as many blocks as the output has tiles where the host knows the total, as many as textCap has where it
	// does not -- the blocks whose tile lies behind *outBytes leave at once
	const uint64_t bytes = std::min(textCap, hostTotal);
	const uint64_t textTiles = bytes && stringTiles ? bytes / kGatTile + 2 : 0;   // (a misaligned outText: one tile more)
	if (textTiles)
		hipLaunchKernelGGL(GatherCopyKernel, dim3(uint32_t(std::min<uint64_t>(textTiles, kGatMaxBlocks))), dim3(kGatThreads), 0, stream, p);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "gather launch");
}

}  // namespace pirehip
