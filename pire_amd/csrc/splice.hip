// The matches of a buffer replaced, the rest kept (pire_hip_splice): from a span list to the rewritten text without leaving
// the device.  The mirror image of gather.hip: the gather keeps the spans and drops the rest, this keeps the rest and puts
// a piece where every span was -- head ++ (the match itself under KEEP) ++ tail --, which is `sed 's/re/repl/g'`, deletion,
// redaction and `grep --color`.  Like the gather it takes no table: any pass that writes ascending byte ranges feeds it.
//
//   k = min(*count, cap)     [b_j, e_j) = span j     P_j = |piece_j| = H + (KEEP ? e_j - b_j : 0) + T
//   G_j = P_j - (e_j - b_j)  D(j) = G_0 + ... + G_{j-1}  (64-bit, wrap-around)     outPos[j] = b_j + D(j)     *outBytes = size + D(k)
//
//   sums      one lane per span: G_j (a span with e_j < b_j counts as empty); one 64-bit sum per tile of 1 024 spans.  The
//             sum of tile t waits in outPos[1024 t], an entry the tile's own first span owns and the positions pass
//             overwrites: where the caller hands outPos in, the pass needs no scratch.
//   scan      exclusive scan of the tile sums, one block, a 64-bit carry between its steps; size + the total is *outBytes.
//   positions every tile reads its base and computes its G_j again: outPos[j] = b_j + tile base + the exclusive scan inside
//             the tile.  With offsets: the tile keeps its b_j and D(j) in LDS, two waves find the strings whose first span
//             lies in the tile (compact.h WaveBound over offsets), and one lane per string finds that span by binary search
//             over the staged b_j: outOffsets[i] = offsets[i] + D(first j with b_j >= offsets[i]).  The strings behind the
//             last span belong to tile k / 1024, which exists for them alone where k is a multiple of 1 024.
//   copy      the work is divided by OUTPUT BYTES.  outText is cut into tiles of 16 KiB on the 16-byte grid of its address;
//             a block finds the pieces that own its tile's first and last byte by search in outPos (compact.h WaveOwner: the
//             owner of byte x is the LAST j with outPos[j] <= x, which steps over the repeated entries that deleted
//             neighbours leave; a byte in front of outPos[0] has no owner and is raw's own), stages their positions and
//             spans in LDS, and then every lane owns 16 output bytes.  It finds its piece by binary search in the staged
//             positions; a group that lies wholly inside kept text -- or, under KEEP, wholly inside a match -- is one
//             unaligned 16-byte load and one 16-byte store (gather.hip's finding: the unaligned load won).  Any other group
//             is assembled run by run: head and tail bytes from LDS, where the block keeps the two strings that arrived as
//             kernel arguments; a run of raw bytes with one unaligned load merged under a byte mask where its 16-byte window
//             lies inside raw, byte by byte where it does not.  A tile of more pieces than the stage holds (1 024: pieces
//             less than 16 bytes apart on average) reads positions and spans from global memory instead.
//
// Every source position is checked against `size` before it is read and every index into the lists stays below k, so a
// list that is not ascending gives unspecified bytes and nothing else.
// Four launches on the caller's stream, the shape of gather.hip: no block waits for another block, no atomics (the output
// is the same bits every time).  Plain HIP with compiler-placed waits: nothing here keeps data on its way in registers.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "compact.h"
#include "internal.h"

namespace pirehip {

namespace {

constexpr uint32_t kSplThreads = kBlockThreads;
constexpr uint32_t kSplWaves = kBlockWaves;
constexpr uint32_t kSplTile = PIRE_HIP_GATHER_TILE_BYTES;   // 16 output bytes a lane
constexpr uint32_t kSplStage = 1024;                        // pieces of a tile kept in LDS: 3 * 8 bytes each
constexpr uint32_t kSplMaxBlocks = 2048;                    // as the gather's: tiles in a grid-stride loop
constexpr uint32_t kSplPiece = PIRE_HIP_SPLICE_PIECE_MAX;   // head and tail: at most this long each
static_assert(kSplTile == kSplThreads * 16, "one dwordx4 per lane and tile");
static_assert(kSplPiece % 4 == 0 && 2 * kSplPiece / 4 <= kSplThreads, "the block copies head and tail into LDS in one step");

struct SpliceParams {
	const uint8_t* raw;
	uint64_t size;
	const uint64_t* spans;
	const uint64_t* count;   // nullable: cap spans
	uint64_t cap;
	uint32_t headLen, tailLen, keep;
	const uint64_t* offsets;   // nullable (with outOffsets)
	uint64_t n;
	uint8_t* outText;
	uint64_t textCap;
	uint64_t* outPos;       // the caller's or the pass's scratch: never null where cap > 0
	uint64_t* outOffsets;
	uint64_t* outBytes;
	uint32_t piece[2 * kSplPiece / 4];   // head from byte 0, tail from byte kSplPiece: they travel as kernel arguments
};

// Where the growth of tile t of the spans waits between the passes (after the scan: the growth in front of the tile)
__device__ __forceinline__ uint64_t* TileSum(const SpliceParams& p, uint64_t tile)
{
	return p.outPos + tile * kSplThreads;
}

__device__ __forceinline__ uint64_t Spans(const SpliceParams& p)
{
	return p.count && p.cap ? std::min(*p.count, p.cap) : p.cap;
}

// Span j as every pass reads it: [*b, *e) with *e >= *b (a span that ends in front of its begin is an empty one)
__device__ __forceinline__ void Span(const SpliceParams& p, uint64_t j, uint64_t* b, uint64_t* e)
{
	*b = p.spans[2 * j];
	*e = std::max(*b, p.spans[2 * j + 1]);
}

// G_j; 0 behind the list
__device__ __forceinline__ uint64_t Growth(const SpliceParams& p, uint64_t j, uint64_t k, uint64_t* b)
{
	*b = ~0ull;
	if (j >= k)
		return 0;
	uint64_t e;
	Span(p, j, b, &e);
	return uint64_t(p.headLen) + p.tailLen - (p.keep ? 0 : e - *b);
}

__global__ __launch_bounds__(kSplThreads) void SpliceSumsKernel(SpliceParams p)
{
	__shared__ uint64_t waveSum[kSplWaves];
	const uint64_t k = Spans(p);
	for (uint64_t base = uint64_t(blockIdx.x) * kSplThreads; base < k; base += uint64_t(gridDim.x) * kSplThreads) {
		uint64_t total, b;
		(void)BlockExclusive(Growth(p, base + threadIdx.x, k, &b), waveSum, &total);
		if (threadIdx.x == 0)
			*TileSum(p, base / kSplThreads) = total;
	}
}

// *TileSum(t) = D(1024 t), *outBytes = size + D(k)
__global__ __launch_bounds__(kSplThreads) void SpliceScanKernel(SpliceParams p)
{
	__shared__ uint64_t waveSum[kSplWaves];
	const uint64_t k = Spans(p);
	const uint64_t tiles = (k + kSplThreads - 1) / kSplThreads;
	uint64_t carry = 0;
	for (uint64_t base = 0; base < tiles; base += kSplThreads) {
		const uint64_t i = base + threadIdx.x;
		const uint64_t v = i < tiles ? *TileSum(p, i) : 0;
		uint64_t total;
		const uint64_t front = BlockExclusive(v, waveSum, &total);
		if (i < tiles)
			*TileSum(p, i) = carry + front;
		carry += total;
	}
	if (threadIdx.x == 0)
		*p.outBytes = p.size + carry;
}

__global__ __launch_bounds__(kSplThreads) void SplicePosKernel(SpliceParams p)
{
	__shared__ uint64_t waveSum[kSplWaves];
	__shared__ uint64_t begins[kSplThreads];      // b_j of the tile's spans, ~0 behind the list
	__shared__ uint64_t grown[kSplThreads + 1];   // D(j) in front of them; [1024]: behind the tile
	__shared__ uint64_t range[2];                 // the strings whose first span lies in the tile
	const uint64_t k = Spans(p);
	// (with offsets: tile k / 1024 is the tile of the strings behind the last span, also where it has no span of its own)
	const uint64_t tiles = p.offsets ? k / kSplThreads + 1 : (k + kSplThreads - 1) / kSplThreads;
	for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
		const uint64_t base = tile * kSplThreads, j = base + threadIdx.x;
		// (read by every lane before the barriers of the scan, written behind them)
		const uint64_t front = base < k ? *TileSum(p, tile) : *p.outBytes - p.size;
		uint64_t total, b;
		const uint64_t g = Growth(p, j, k, &b);
		const uint64_t d = front + BlockExclusive(g, waveSum, &total);
		if (j < k)
			p.outPos[j] = b + d;
		if (!p.offsets)
			continue;
		begins[threadIdx.x] = b;
		grown[threadIdx.x] = d;
		if (threadIdx.x == 0)
			grown[kSplThreads] = front + total;
		const uint32_t wave = threadIdx.x >> 6;
		if (wave < 2) {
			// string i is the tile's where b_{base - 1} < offsets[i] <= b_{base + 1023}: counts of offsets[0, n] <= a begin
			uint64_t r;
			if (wave == 0)
				r = tile == 0 ? 0 : WaveBound<true>(p.offsets, p.n + 1, LoadU64(p.spans, 2 * (base - 1)));
			else
				r = base + kSplThreads > k ? p.n + 1 : WaveBound<true>(p.offsets, p.n + 1, LoadU64(p.spans, 2 * (base + kSplThreads - 1)));
			if ((threadIdx.x & 63) == 0)
				range[wave] = r;
		}
		__syncthreads();
		const uint32_t m = uint32_t(std::min<uint64_t>(k - base, kSplThreads));
		for (uint64_t i = range[0] + threadIdx.x; i < range[1]; i += kSplThreads) {
			const uint64_t x = p.offsets[i];
			uint32_t lo = 0, hi = m;   // the first staged span with b_j >= x; m: none, the string begins behind them all
			while (lo < hi) {
				const uint32_t mid = (lo + hi) / 2;
				if (begins[mid] >= x)
					hi = mid;
				else
					lo = mid + 1;
			}
			p.outOffsets[i] = x + grown[lo];
		}
		__syncthreads();   // (the next tile writes the stage again)
	}
}

// The tile's pieces s0 .. s0 + m - 1 as a lane reads them: where piece i begins in the output, and its span
struct StagedPieces {
	const uint64_t *pos, *b, *e;
	__device__ __forceinline__ uint64_t Pos(uint32_t i) const { return pos[i]; }
	__device__ __forceinline__ void Range(uint32_t i, uint64_t* begin, uint64_t* end) const { *begin = b[i], *end = e[i]; }
};
struct DirectPieces {
	const SpliceParams& p;
	uint64_t s0;
	__device__ __forceinline__ uint64_t Pos(uint32_t i) const { return p.outPos[s0 + i]; }
	__device__ __forceinline__ void Range(uint32_t i, uint64_t* begin, uint64_t* end) const { Span(p, s0 + i, begin, end); }
};

struct __attribute__((packed, aligned(1))) Unaligned16 {
	uint32_t w[4];
};

// 0xFF in bytes [from, to) of dword k of a 16-byte group, 0 <= from <= to <= 16
__device__ __forceinline__ uint32_t ByteMask(uint32_t k, uint32_t from, uint32_t to)
{
	const uint32_t a = std::min(std::max(from, 4 * k), 4 * k + 4) - 4 * k, b = std::min(std::max(to, 4 * k), 4 * k + 4) - 4 * k;   // 0..4
	const uint32_t below = b == 4 ? 0xFFFFFFFFu : (1u << (8 * b)) - 1, under = a == 4 ? 0xFFFFFFFFu : (1u << (8 * a)) - 1;
	return below & ~under;
}

// Byte i of the group = v (selects, no indexing: w stays in registers)
__device__ __forceinline__ void PutByte(uint32_t (&w)[4], uint32_t i, uint32_t v)
{
	const uint32_t shift = 8 * (i & 3);
#pragma unroll
	for (uint32_t k = 0; k < 4; ++k)
		w[k] = (i >> 2) == k ? (w[k] & ~(0xFFu << shift)) | (v << shift) : w[k];
}

// Bytes [from, to) of the group = raw[src, src + to - from): one unaligned load of the 16-byte window around them where that
// window lies inside raw, else byte by byte -- and 0 for a position that is not raw's (a list that breaks the promise)
__device__ __forceinline__ void MergeRaw(const SpliceParams& p, uint64_t src, uint32_t from, uint32_t to, uint32_t (&w)[4])
{
	const uint64_t window = src - from;
	if (src >= from && p.size >= 16 && window <= p.size - 16) {
		const Unaligned16 q = *reinterpret_cast<const Unaligned16*>(p.raw + window);
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k) {
			const uint32_t mask = ByteMask(k, from, to);
			w[k] = (w[k] & ~mask) | (q.w[k] & mask);
		}
	} else {
		for (uint32_t i = from; i < to; ++i) {
			const uint64_t at = src + (i - from);
			PutByte(w, i, at < p.size ? p.raw[at] : 0);
		}
	}
}

// The lane's output bytes [lo, hi) -- a whole 16-byte group of outText's grid, or the part of one that lies inside
// [0, limit) -- out of the m pieces of the tile.  piece: head from byte 0, tail from byte kSplPiece (LDS).
template <class Pieces>
__device__ __forceinline__ void CopyLane(const SpliceParams& p, const Pieces& s, uint32_t m, const uint8_t* piece, uint64_t lo, uint64_t hi)
{
	uint32_t at = 0, end = m;   // how many of the tile's pieces begin at or in front of lo
	while (at < end) {
		const uint32_t mid = (at + end) / 2;
		if (s.Pos(mid) <= lo)
			at = mid + 1;
		else
			end = mid;
	}
	// the piece that owns lo: none (at == 0) is an empty piece at 0 that replaces nothing -- kept text from raw[0] behind it
	uint64_t pos = 0, b = 0, e = 0;
	uint32_t H = 0, T = 0;
	if (at > 0) {
		pos = s.Pos(at - 1);
		s.Range(at - 1, &b, &e);
		H = p.headLen, T = p.tailLen;
	}
	uint64_t next = at < m ? s.Pos(at) : ~0ull;   // (the piece behind the tile's last begins behind the tile)
	uint32_t w[4] = {0, 0, 0, 0};
	bool done = false;
	if (hi - lo == 16 && next >= hi && lo >= pos) {
		const uint64_t off = lo - pos, mid = p.keep ? e - b : 0, len = H + mid + T;
		uint64_t src = ~0ull;
		if (off >= len)
			src = e + (off - len);            // kept text
		else if (off >= H && off + 16 <= H + mid)
			src = b + (off - H);              // inside the match itself
		if (p.size >= 16 && src <= p.size - 16) {
			const Unaligned16 q = *reinterpret_cast<const Unaligned16*>(p.raw + src);
			w[0] = q.w[0], w[1] = q.w[1], w[2] = q.w[2], w[3] = q.w[3];
			done = true;
		}
	}
	if (!done) {
		const uint32_t bytes = uint32_t(hi - lo);   // 1..16; byte i of the lane is output position lo + i
		uint32_t i = 0;
		while (i < bytes) {
			const uint64_t x = lo + i;
			while (at < m && next <= x) {   // (empty pieces in between)
				pos = next;
				s.Range(at, &b, &e);
				H = p.headLen, T = p.tailLen;
				++at;
				next = at < m ? s.Pos(at) : ~0ull;
			}
			const uint64_t off = x - pos, mid = p.keep ? e - b : 0, len = H + mid + T;
			const uint64_t room = std::max<uint64_t>(std::min<uint64_t>(next - x, bytes - i), 1);   // up to the next piece or the group's end
			uint32_t run;
			if (off < H) {
				run = uint32_t(std::min<uint64_t>(room, H - off));
				for (uint32_t q = 0; q < run; ++q)
					PutByte(w, i + q, piece[uint32_t(off) + q]);
			} else if (off < H + mid) {
				run = uint32_t(std::min<uint64_t>(room, H + mid - off));
				MergeRaw(p, b + (off - H), i, i + run, w);
			} else if (off < len) {
				run = uint32_t(std::min<uint64_t>(room, len - off));
				for (uint32_t q = 0; q < run; ++q)
					PutByte(w, i + q, piece[kSplPiece + uint32_t(off - H - mid) + q]);
			} else {
				run = uint32_t(room);
				MergeRaw(p, e + (off - len), i, i + run, w);
			}
			i += run;
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

__global__ __launch_bounds__(kSplThreads) void SpliceCopyKernel(SpliceParams p)
{
	__shared__ uint64_t pos[kSplStage], begin[kSplStage], end[kSplStage];
	__shared__ uint32_t piece[2 * kSplPiece / 4];
	__shared__ uint64_t owner[2];
	if (threadIdx.x < 2 * kSplPiece / 4)
		piece[threadIdx.x] = p.piece[threadIdx.x];
	const uint64_t k = Spans(p);
	const uint64_t limit = std::min(*p.outBytes, p.textCap);   // output bytes [0, limit) are written
	// outText's address modulo 16: tiles and groups are counted from the 16-byte boundary in front of it
	const uint64_t head = reinterpret_cast<uintptr_t>(p.outText) & 15;
	const uint64_t tiles = limit ? (head + limit + kSplTile - 1) / kSplTile : 0;
	for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
		const uint64_t tileLo = std::max(tile * kSplTile, head) - head;                 // output positions
		const uint64_t tileHi = std::min((tile + 1) * kSplTile, head + limit) - head;   // tileLo < tileHi <= limit
		const uint32_t wave = threadIdx.x >> 6;
		if (wave < 2) {
			const uint64_t o = WaveOwner(p.outPos, k, wave == 0 ? tileLo : tileHi - 1);   // (0 also where no piece owns the byte)
			if ((threadIdx.x & 63) == 0)
				owner[wave] = o;
		}
		__syncthreads();   // (and piece is written)
		const uint64_t s0 = owner[0];
		const uint64_t count = k ? std::max(owner[1], s0) - s0 + 1 : 0;   // (the max: a list that is not ascending)
		const bool staged = count <= kSplStage;
		const uint32_t m = uint32_t(count);   // (k < 2^32)
		if (staged) {
			for (uint32_t i = threadIdx.x; i < m; i += kSplThreads) {
				pos[i] = p.outPos[s0 + i];
				Span(p, s0 + i, &begin[i], &end[i]);
			}
			__syncthreads();
		}
		const uint64_t v = tile * kSplTile + threadIdx.x * 16;   // the lane's group, on outText's grid
		const uint64_t lo = std::max(v, head) - head;
		const uint64_t hi = std::min(v + 16, head + limit) - head;   // (v + 16 > head: head < 16)
		if (lo < hi) {
			if (staged)
				CopyLane(p, StagedPieces{pos, begin, end}, m, reinterpret_cast<const uint8_t*>(piece), lo, hi);
			else
				CopyLane(p, DirectPieces{p, s0}, m, reinterpret_cast<const uint8_t*>(piece), lo, hi);
		}
		__syncthreads();   // (the next tile writes owner and the stage again)
	}
}

}  // namespace

int LaunchSplice(const void* raw, uint64_t size, const uint64_t* spans, const uint64_t* count, uint64_t cap, const void* head, uint32_t headLen,
                 const void* tail, uint32_t tailLen, uint32_t mode, const uint64_t* offsets, uint64_t n, void* outText, uint64_t textCap,
                 uint64_t* outPos, uint64_t* outOffsets, uint64_t* outBytes, uint64_t hostTotal, hipStream_t stream)
{
	SpliceParams p = {};
	p.raw = static_cast<const uint8_t*>(raw);
	p.size = size;
	p.spans = spans;
	p.count = count;
	p.cap = cap;
	p.headLen = headLen;
	p.tailLen = tailLen;
	p.keep = (mode & PIRE_HIP_SPLICE_KEEP) != 0;
	p.offsets = outOffsets ? offsets : nullptr;
	p.n = n;
	p.outText = static_cast<uint8_t*>(outText);
	p.textCap = textCap;
	p.outPos = outPos;
	p.outOffsets = outOffsets;
	p.outBytes = outBytes;
	if (headLen)
		memcpy(p.piece, head, headLen);
	if (tailLen)
		memcpy(reinterpret_cast<uint8_t*>(p.piece) + kSplPiece, tail, tailLen);
	const uint64_t spanTiles = (cap + kSplThreads - 1) / kSplThreads;
	const uint64_t posTiles = p.offsets ? cap / kSplThreads + 1 : spanTiles;
	if (spanTiles)
		hipLaunchKernelGGL(SpliceSumsKernel, dim3(uint32_t(std::min<uint64_t>(spanTiles, kSplMaxBlocks))), dim3(kSplThreads), 0, stream, p);
	hipLaunchKernelGGL(SpliceScanKernel, dim3(1), dim3(kSplThreads), 0, stream, p);
	if (posTiles)
		hipLaunchKernelGGL(SplicePosKernel, dim3(uint32_t(std::min<uint64_t>(posTiles, kSplMaxBlocks))), dim3(kSplThreads), 0, stream, p);
	// the copy pass: as many blocks as the output has tiles where the host knows the total, as many as the largest output has
	// where it does not (every piece at most headLen + tailLen longer than its span) -- the blocks behind *outBytes leave at once
	const uint64_t most = hostTotal != kSpliceTotalUnknown ? hostTotal : size + cap * (uint64_t(headLen) + tailLen);
	const uint64_t bytes = std::min(textCap, most);
	if (bytes)   // (a misaligned outText: one tile more)
		hipLaunchKernelGGL(SpliceCopyKernel, dim3(uint32_t(std::min<uint64_t>(bytes / kSplTile + 2, kSplMaxBlocks))), dim3(kSplThreads), 0, stream, p);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "splice launch");
}

}  // namespace pirehip
