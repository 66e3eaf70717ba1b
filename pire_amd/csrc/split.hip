// Raw text into strings on the device (pire_hip_split): where the lines of a buffer are.
//
// Every scan entry point takes text + offsets[n + 1], the strings back to back with nothing between them.  What a caller
// has is a file or a network buffer with a delimiter byte between the lines; cutting it on one host core (find, append,
// push_back: examples/pigrep_hip.cpp did just that) runs at memchr speed in front of a scan that runs at TB/s.  This unit
// does the cut where the scan is.  getline's semantics: the strings are the runs between delimiter bytes, the delimiter
// is not part of a string, a trailing fragment without a delimiter is a string, a buffer that ends in a delimiter has no
// extra empty string behind it, consecutive delimiters give empty strings.  With D delimiters at p_1 < ... < p_D:
//
//   n = D + (size > 0 && raw[size - 1] != delim)      offsets[0] = 0      offsets[k] = p_k - (k - 1)      offsets[n] = size - D
//   out_text = raw without its delimiter bytes        =>  line i is raw[offsets[i] + i, offsets[i + 1] + i)
//
//   count     raw is cut into tiles of 16 KiB ON THE 16-BYTE GRID OF ITS ADDRESS (a misaligned raw has a short first tile):
//             a lane loads its 16 bytes with one global_load_dwordx4 (compact.h LoadLane) -- the lanes that hang over the buffer's two ends load
//             their bytes one by one --, compares them with the delimiter (a 16-bit mask), popcounts; one count per tile.
//   scan      exclusive scan of the tile counts, one block, 1 024 tiles (16 MiB of text) a step, a 64-bit carry between the
//             steps; the total and the trailing-fragment term are *out_n.
//   scatter   every tile counts again; the rank of a delimiter = tile prefix + the waves and lanes in front + its rank in the
//             lane's mask -> offsets[rank + 1].  The bytes that stay move to out_text[pos - rank(pos)]: staged in LDS at a
//             local position CONGRUENT MOD 16 TO THEIR ADDRESS in out_text, so that the tile's output leaves as whole
//             16-byte groups (global_store_dwordx4); only the partial groups at the tile's two ends go out by bytes (the
//             neighbouring tiles own the other bytes of those groups).  A lane without a delimiter -- nearly every lane on
//             real lines -- moves its 16 bytes into LDS as three realigned dwords (funnel shifts) + at most four single bytes;
//             a lane with one compacts byte by byte.
//
// Three launches on the caller's stream, the shape of select.hip and order.hip: no block waits for another block, no
// atomics (the output is the same bits every time), scratch (12 bytes per tile) from the stream-ordered allocator.  With
// out_text == NULL nothing is copied and the strings keep their delimiters: offsets[k] = p_k + 1, indices into raw itself.
// Plain HIP with compiler-placed waits: nothing here keeps data on its way in registers.
//
// pire_hip_run_lines_select (api.cpp) splits into scratch, scans, selects, and SplitSpansKernel turns the hit list into
// byte ranges of the raw buffer -- and the R hit lists of pire_hip_run_lines_route, in one launch (LaunchHitSpans).  The
// block-wide prefix sum of the three kernels is compact.h's BlockExclusive.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "compact.h"
#include "internal.h"

namespace pirehip {

namespace {

constexpr uint32_t kSplitThreads = kBlockThreads;
constexpr uint32_t kSplitWaves = kBlockWaves;
constexpr uint32_t kSplitTile = PIRE_HIP_SPLIT_TILE_BYTES;   // 16 bytes a lane
constexpr uint32_t kSplitMaxBlocks = 2048;                   // 2 blocks on each of 256 CUs, four rounds; tiles in a grid-stride loop
static_assert(kSplitTile == kSplitThreads * 16, "one dwordx4 per lane and tile");

__global__ __launch_bounds__(kSplitThreads) void SplitCountKernel(SplitPlan p)
{
	__shared__ uint32_t waveSum[kSplitWaves];
	for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
		uint32_t w[4], valid, total;
		const uint32_t dm = LoadLane(p.raw, p.head, p.size, p.delim4, uint64_t(tile) * kSplitTile + threadIdx.x * 16, w, &valid);
		(void)BlockExclusive(uint32_t(__popc(dm)), waveSum, &total);
		if (threadIdx.x == 0)
			p.counts[tile] = total;
	}
}

// prefix[t] = delimiters in front of tile t (64 bits: a buffer may hold more than 2^32), *outN = the number of strings
__global__ __launch_bounds__(kSplitThreads) void SplitScanKernel(SplitPlan p, uint64_t* outN)
{
	__shared__ uint32_t waveSum[kSplitWaves];
	uint64_t carry = 0;
	for (uint32_t base = 0; base < p.tiles; base += kSplitThreads) {
		const uint32_t i = base + threadIdx.x;
		uint32_t total;
		const uint32_t front = BlockExclusive(i < p.tiles ? p.counts[i] : 0, waveSum, &total);   // (a step's total: 2^24 at most)
		if (i < p.tiles)
			p.prefix[i] = carry + front;
		carry += total;
	}
	if (threadIdx.x == 0) {
		const bool fragment = p.size && p.raw[p.size - 1] != (p.delim4 & 0xFFu);
		*outN = carry + (fragment ? 1 : 0);
	}
}

// kCopy: the bytes that are not delimiters go to outText; otherwise the strings keep their delimiters and stay where they are
template <bool kCopy>
__global__ __launch_bounds__(kSplitThreads) void SplitScatterKernel(SplitPlan p, uint8_t* outText, uint64_t* offsets, uint64_t cap,
                                                                    const uint64_t* outN)
{
	__shared__ uint32_t waveSum[kSplitWaves];
	__shared__ __attribute__((aligned(16))) uint8_t stage[kCopy ? kSplitTile + 16 : 16];
	const uint64_t end = p.head + p.size;
	if (offsets && blockIdx.x == 0 && threadIdx.x == 0) {
		// the two entries no delimiter stands for: the first, and the one behind a trailing fragment
		const uint64_t n = *outN;
		const bool fragment = p.size && p.raw[p.size - 1] != (p.delim4 & 0xFFu);
		offsets[0] = 0;
		if (fragment && n <= cap)
			offsets[n] = kCopy ? p.size - (n - 1) : p.size;
	}
	// outText's address modulo 16: output positions are counted from the 16-byte boundary in front of it
	const uint32_t outHead = kCopy ? uint32_t(reinterpret_cast<uintptr_t>(outText) & 15) : 0;
	for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
		const uint64_t v = uint64_t(tile) * kSplitTile + threadIdx.x * 16;
		uint32_t w[4], valid, total;
		const uint32_t dm = LoadLane(p.raw, p.head, p.size, p.delim4, v, w, &valid);
		const uint32_t front = BlockExclusive(uint32_t(__popc(dm)), waveSum, &total);
		const uint64_t tilePrefix = p.prefix[tile];
		const uint64_t rank0 = tilePrefix + front;   // delimiters in front of this lane's bytes
		if (offsets)
			for (uint32_t m = dm; m; m &= m - 1) {
				const uint32_t b = uint32_t(__ffs(int(m))) - 1;
				const uint64_t rank = rank0 + uint32_t(__popc(dm & ((1u << b) - 1)));
				const uint64_t pos = v + b - p.head;
				if (rank < cap)
					offsets[rank + 1] = kCopy ? pos - rank : pos + 1;
			}
		if (kCopy) {
			const uint64_t tileLo = std::max<uint64_t>(uint64_t(tile) * kSplitTile, p.head);
			const uint64_t tileHi = std::min<uint64_t>(uint64_t(tile + 1) * kSplitTile, end);
			const uint64_t out0 = outHead + (tileLo - p.head) - tilePrefix;           // where the tile's output begins ...
			const uint64_t out1 = outHead + (tileHi - p.head) - tilePrefix - total;   // ... and ends
			const uint64_t group0 = out0 & ~uint64_t(15);
			if (valid) {
				uint32_t l = uint32_t(outHead + (std::max<uint64_t>(v, p.head) - p.head) - rank0 - group0);
				if (dm == 0 && valid == 0xFFFFu) {
					const uint32_t head = (4 - (l & 3)) & 3;   // single bytes up to the next dword of LDS, as many behind the three dwords
					if (head == 0) {
						uint32_t* d = reinterpret_cast<uint32_t*>(stage + l);
						d[0] = w[0], d[1] = w[1], d[2] = w[2], d[3] = w[3];
					} else {
#pragma unroll
						for (uint32_t i = 0; i < 3; ++i)
							if (i < head)
								stage[l + i] = uint8_t(w[0] >> (8 * i));
						uint32_t* d = reinterpret_cast<uint32_t*>(stage + l + head);
#pragma unroll
						for (uint32_t k = 0; k < 3; ++k)
							d[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], head);   // bytes head .. head + 3 of the pair
						const uint32_t last = w[3] >> (8 * head);
#pragma unroll
						for (uint32_t i = 0; i < 3; ++i)
							if (i < 4 - head)
								stage[l + head + 12 + i] = uint8_t(last >> (8 * i));
					}
				} else {
					const uint32_t keep = valid & ~dm;
#pragma unroll
					for (uint32_t i = 0; i < 16; ++i)
						if ((keep >> i) & 1)
							stage[l++] = uint8_t(w[i >> 2] >> (8 * (i & 3)));
				}
			}
			__syncthreads();
			const uint32_t lo = uint32_t(out0 - group0), hi = uint32_t(out1 - group0);   // lo < 16, lo <= hi <= lo + 16 KiB
			uint8_t* dst = outText + ptrdiff_t(group0 - outHead);   // 16-byte aligned
			for (uint32_t g = threadIdx.x * 16; g < hi; g += kSplitTile) {
				const uint32_t s0 = std::max(g, lo), s1 = std::min(g + 16, hi);
				if (s0 == g && s1 == g + 16)
					*reinterpret_cast<uint4*>(dst + g) = *reinterpret_cast<const uint4*>(stage + g);
				else
					for (uint32_t s = s0; s < s1; ++s)
						dst[s] = stage[s];
			}
			__syncthreads();
		}
	}
}

// The spans of the hit lists hits[rows][pitch]: hit k of row r is line i = hits[r][k], the bytes raw[offsets[i] + i,
// offsets[i + 1] + i) of the raw buffer (offsets: of the text without its delimiters), for k < min(counts[r], kMax).  One
// list (the select pass's): rows = 1, pitch = kMax = its capacity; the route pass's R rows in the same launch, over (r, k).
__global__ void SplitSpansKernel(const uint64_t* hits, const uint64_t* counts, uint32_t rows, uint64_t pitch, uint64_t kMax,
                                 const uint64_t* offsets, uint64_t* spans)
{
	const uint64_t k = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y)
		if (k < kMax && k < counts[r]) {
			const uint64_t at = uint64_t(r) * pitch + k;
			const uint64_t i = hits[at];
			spans[2 * at] = offsets[i] + i;
			spans[2 * at + 1] = offsets[i + 1] + i;
		}
}

}  // namespace

int LaunchSplitCount(const void* raw, uint64_t size, uint32_t delim, uint64_t* outN, hipStream_t stream, StreamScratch& scratch,
                     SplitPlan* plan)
{
	SplitPlan& p = *plan;
	const uintptr_t addr = reinterpret_cast<uintptr_t>(raw);
	p.raw = static_cast<const uint8_t*>(raw);
	p.head = size ? uint32_t(addr & 15) : 0;
	p.size = size;
	p.delim4 = (delim & 0xFFu) * 0x01010101u;
	const uint64_t tiles = (p.head + size + kSplitTile - 1) / kSplitTile;
	if (tiles >= (1ull << 32)) {
		SetError("pire_hip_split: 2^32 tiles of 16 KiB or more in one call");
		return PIRE_HIP_EUNSUPPORTED;
	}
	p.tiles = uint32_t(tiles);
	if (int rc = scratch.Alloc(size_t(tiles) * 12 + 16, "hipMallocAsync(split scratch)"))
		return rc;
	p.prefix = scratch.as<uint64_t>();
	p.counts = reinterpret_cast<uint32_t*>(p.prefix + tiles);
	if (p.tiles)
		hipLaunchKernelGGL(SplitCountKernel, dim3(std::min(p.tiles, kSplitMaxBlocks)), dim3(kSplitThreads), 0, stream, p);
	hipLaunchKernelGGL(SplitScanKernel, dim3(1), dim3(kSplitThreads), 0, stream, p, outN);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "split launch");
}

int LaunchSplitScatter(const SplitPlan& p, void* outText, uint64_t* outOffsets, uint64_t offsetsCap, const uint64_t* outN,
                       hipStream_t stream)
{
	if (!outText && !outOffsets)
		return PIRE_HIP_OK;
	const dim3 grid(std::max(1u, std::min(p.tiles, kSplitMaxBlocks)));   // (an empty buffer still gets its offsets[0])
	if (outText)
		hipLaunchKernelGGL(SplitScatterKernel<true>, grid, dim3(kSplitThreads), 0, stream, p, static_cast<uint8_t*>(outText), outOffsets,
		                   offsetsCap, outN);
	else
		hipLaunchKernelGGL(SplitScatterKernel<false>, grid, dim3(kSplitThreads), 0, stream, p, nullptr, outOffsets, offsetsCap, outN);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "split launch");
}

int LaunchHitSpans(const uint64_t* hits, const uint64_t* counts, uint32_t rows, uint64_t pitch, uint64_t kMax, const uint64_t* offsets,
                   uint64_t* spans, hipStream_t stream, const char* what)
{
	if (!kMax || !rows)
		return PIRE_HIP_OK;
	const dim3 grid(uint32_t((kMax + 255) / 256), std::min(rows, 65535u));
	hipLaunchKernelGGL(SplitSpansKernel, grid, dim3(256), 0, stream, hits, counts, rows, pitch, kMax, offsets, spans);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, what);
}

}  // namespace pirehip
