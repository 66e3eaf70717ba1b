// From end states to matches on the device (pire_hip_select): which strings matched which regexps.
//
// Every scan entry point answers with one StateIndex per string.  What a caller of a multi-regexp scanner wants is the
// set of regexps that state accepts (AcceptedRegexps, multi.h:149-158) and, usually, only the strings that matched at
// all -- a compacted, ascending list of their indices.  This unit turns the one into the other without leaving the
// device, behind ANY of the scan kernels (it reads state indices, nothing else of a scan):
//
//   image     per state, by REFERENCE state index: W = max(1, ceil(regexps / 64)) mask words and the Final flag
//             (internal.h SelectHost).  Reference numbering, so no re-ranking ever touches it.
//   classify  one lane per string: state index -> mask record -> selected?  The masks go out if asked for; the selected
//             bits of a wave are one ballot word, kept in scratch; one count per tile of 1 024 strings.
//   scan      exclusive scan of the tile counts, one block a row of them (one row here; capture_select.hip's one and
//             route.hip's R rows go through the same kernel, LaunchTileScan); the total is the hit count.
//   scatter   rank of a selected string = tile offset + the popcounts of the waves in front + mbcnt of its own wave's
//             ballot word: the hits come out in ascending order, deterministically, with no atomics.
//
// The block scan and the classify tail are compact.h's (BlockExclusive, TileBallot); the scatter kernel and the launcher are
// tile_pass.h's, shared with the seven passes that came after this one.  This unit also defines what they all call on the
// host: the tile scan (LaunchTileScan), the launcher's front (TileCompaction) and the staging of a count and its lists (HitStage).
// Three launches on the caller's stream, the shape of order.hip.  No block ever waits for another block (no look-back,
// no flags between blocks): the order of the three kernels on the stream is the only synchronisation.
//
// The gather is 8 * W bytes per string from a table of a few hundred KiB at most (L2 resident).  For W == 1 and up to
// 8 192 states a block that has enough tiles to pay for it copies the table to LDS first: one ds_read_b64 per lane.
// Plain HIP with compiler-placed waits: nothing here keeps data on its way in registers.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "tile_pass.h"

namespace pirehip {

namespace {

constexpr uint32_t kSelScanBlocks = 1024;          // the tile scan's grid: a block per row, rows in a grid-stride loop
constexpr uint32_t kSelLdsStates = 8192;           // x 8 bytes = 64 KiB: two blocks a CU
constexpr uint32_t kSelLdsBlocks = 512;            // the LDS form's grid: 2 blocks on each of 256 CUs, tiles in a grid-stride loop

struct SelectPass {
	const uint64_t* masks;   // [states * words], reference numbering
	const uint8_t* fin;      // [states]
	uint32_t states, words;
	const uint32_t* stateIdx;
	uint64_t n;
	const uint64_t* want;    // nullable: [words]
	uint64_t* outMasks;      // nullable
	uint32_t store16;        // outMasks is 16-byte aligned and words is even: pairs of words in one store
	uint64_t* outHits;
	uint64_t* outHitMasks;   // nullable

	__device__ __forceinline__ void Write(uint64_t rank, uint64_t i) const
	{
		outHits[rank] = i;
		if (outHitMasks) {
			const uint32_t s = stateIdx[i];
			for (uint32_t w = 0; w < words; ++w)
				outHitMasks[rank * words + w] = s < states ? masks[size_t(s) * words + w] : 0;
		}
	}
};

// A state index beyond the table (undefined behaviour of the ON_DEVICE form; the host-pointer form refuses it) reads
// nothing: an empty mask, not selected.
template <bool kLds>
__global__ __launch_bounds__(kBlockThreads) void SelectClassifyKernel(SelectPass p, TileScratch t)
{
	extern __shared__ uint64_t ldsMasks[];
	__shared__ uint32_t waveCount[kBlockWaves];
	if (kLds) {
		for (uint32_t s = threadIdx.x; s < p.states; s += kBlockThreads)
			ldsMasks[s] = p.masks[s];
		__syncthreads();
	}
	const bool needMask = p.want || p.outMasks;
	for (uint32_t tile = blockIdx.x; tile < t.tiles; tile += gridDim.x) {
		const uint64_t i = uint64_t(tile) * kBlockThreads + threadIdx.x;
		bool sel = false;
		if (i < p.n) {
			const uint32_t s = p.stateIdx[i];
			const bool known = s < p.states;
			if (!p.want)
				sel = known && p.fin[s] != 0;
			if (needMask) {
				if (kLds || p.words == 1) {
					const uint64_t m = !known ? 0 : kLds ? ldsMasks[s] : p.masks[s];
					if (p.want)
						sel = (m & p.want[0]) != 0;
					if (p.outMasks)
						p.outMasks[i] = m;
				} else if (p.store16) {
					const ulonglong2* rec = reinterpret_cast<const ulonglong2*>(p.masks + size_t(s) * p.words);
					ulonglong2* out = reinterpret_cast<ulonglong2*>(p.outMasks + i * p.words);
					uint64_t any = 0;
					for (uint32_t w = 0; w < p.words; w += 2) {
						ulonglong2 m = known ? rec[w / 2] : make_ulonglong2(0, 0);
						if (p.want)
							any |= (m.x & p.want[w]) | (m.y & p.want[w + 1]);
						out[w / 2] = m;
					}
					if (p.want)
						sel = any != 0;
				} else {
					uint64_t any = 0;
					for (uint32_t w = 0; w < p.words; ++w) {
						const uint64_t m = known ? p.masks[size_t(s) * p.words + w] : 0;
						if (p.want)
							any |= m & p.want[w];
						if (p.outMasks)
							p.outMasks[i * p.words + w] = m;
					}
					if (p.want)
						sel = any != 0;
				}
			}
		}
		TileBallot(sel, tile, t.ballots, t.tileCounts, waveCount);
	}
}

// The tile scan of every hit pass (the eight ballot compactions through tile_pass.h, route.hip): exclusive scan of every row of
// counts[rows][entries] in place, a block per row (grid-stride): 1 024 entries (2^20 strings) a step, a carry between the
// steps.  A batch of 2^20 strings is one step; 2^24 strings, sixteen.  outCounts[r] = the total of row r.
__global__ __launch_bounds__(kBlockThreads) void SelectScanKernel(uint32_t* counts, uint32_t rows, uint32_t entries, uint64_t* outCounts)
{
	__shared__ uint32_t waveSum[kBlockWaves];
	for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
		uint32_t* row = counts + size_t(r) * entries;
		uint32_t carry = 0;
		for (uint32_t base = 0; base < entries; base += kBlockThreads) {
			const uint32_t i = base + threadIdx.x;
			uint32_t total;
			const uint32_t front = BlockExclusive(i < entries ? row[i] : 0, waveSum, &total);
			if (i < entries)
				row[i] = carry + front;
			carry += total;
		}
		if (threadIdx.x == 0)
			outCounts[r] = carry;
	}
}

void FreeSelectDevice(SelectDevice* d)
{
	if (d->masks) (void)hipFree(d->masks);
	if (d->fin) (void)hipFree(d->fin);
	*d = SelectDevice();
}

void BuildSelectHost(const HostTable& h, SelectHost& s)
{
	s.words = SelectMaskWords(h.regexps);
	s.masks.assign(size_t(h.states) * s.words, 0);
	s.fin.assign(h.states, 0);
	for (uint32_t st = 0; st < h.states; ++st) {
		for (uint64_t k = h.acceptOff[st]; k < h.acceptOff[st + 1]; ++k) {
			const uint64_t r = h.acceptIds[k];
			if (r < h.regexps)
				s.masks[size_t(st) * s.words + r / 64] |= uint64_t(1) << (r % 64);
		}
		// (a scanner without regexps selects nothing, whatever its flags say)
		s.fin[st] = h.regexps && (h.flags[st] & kFinal) ? 1 : 0;
	}
	s.built = true;
}

}  // namespace

uint32_t SelectMaskWords(uint32_t regexps)
{
	return std::max<uint32_t>(1, (regexps + 63) / 64);
}

void FreeSelect(pire_hip_table* t)
{
	int cur = -1;
	(void)hipGetDevice(&cur);
	for (int k = 0; k < kMaxDevices; ++k)
		if (t->selectDev[k].device >= 0) {
			(void)hipSetDevice(k);
			FreeSelectDevice(&t->selectDev[k]);
		}
	if (cur >= 0)
		(void)hipSetDevice(cur);
}

int UploadSelect(pire_hip_table* t, SelectDevice* image)
{
	int dev = 0;
	hipError_t e = hipGetDevice(&dev);
	if (e != hipSuccess)
		return HipFail(e, "hipGetDevice");
	if (dev < 0 || dev >= kMaxDevices) {
		SetError("device number out of range");
		return PIRE_HIP_EUNSUPPORTED;
	}
	std::lock_guard<std::mutex> lock(t->selectMutex);
	if (!t->select.built)
		BuildSelectHost(t->host, t->select);
	const SelectHost& h = t->select;
	SelectDevice& d = t->selectDev[dev];
	if (d.device != dev) {
		// (16 bytes of slack: an empty table still gets two valid pointers)
		e = hipMalloc(reinterpret_cast<void**>(&d.masks), h.masks.size() * 8 + 16);
		if (e == hipSuccess && !h.masks.empty())
			e = hipMemcpy(d.masks, h.masks.data(), h.masks.size() * 8, hipMemcpyHostToDevice);
		if (e == hipSuccess)
			e = hipMalloc(reinterpret_cast<void**>(&d.fin), h.fin.size() + 16);
		if (e == hipSuccess && !h.fin.empty())
			e = hipMemcpy(d.fin, h.fin.data(), h.fin.size(), hipMemcpyHostToDevice);
		if (e != hipSuccess) {
			FreeSelectDevice(&d);
			return HipFail(e, "uploading the select image");
		}
		d.device = dev;
	}
	if (image)
		*image = d;
	return PIRE_HIP_OK;
}

void LaunchTileScan(uint32_t* counts, uint32_t rows, uint32_t entries, uint64_t* outCounts, hipStream_t stream)
{
	hipLaunchKernelGGL(SelectScanKernel, dim3(std::min(rows, kSelScanBlocks)), dim3(kBlockThreads), 0, stream, counts, rows, entries, outCounts);
}

int TileCompaction(const char* who, const char* scratchLabel, uint64_t n, uint64_t* outHitCount, hipStream_t stream, StreamScratch& scratch,
                   TileScratch* s)
{
	*s = TileScratch();
	if (n == 0) {
		const hipError_t e = hipMemsetAsync(outHitCount, 0, 8, stream);
		return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemsetAsync(hit count)");
	}
	if (n >= (1ull << 32)) {
		SetError(std::string(who) + ": 2^32 strings or more in one call");   // tile offsets are 32 bits (as order.hip's indices)
		return PIRE_HIP_EUNSUPPORTED;
	}
	const uint32_t t = uint32_t((n + kBlockThreads - 1) / kBlockThreads);
	// scratch: n / 8 bytes of ballot words + n / 256 bytes of tile counts, stream-ordered (the call only enqueues)
	const size_t ballotBytes = size_t(t) * kBlockWaves * 8;
	if (int rc = scratch.Alloc(ballotBytes + size_t(t) * 4, scratchLabel))
		return rc;
	s->ballots = scratch.as<uint64_t>();
	s->tileCounts = reinterpret_cast<uint32_t*>(scratch.as<uint8_t>() + ballotBytes);
	s->tiles = t;
	return PIRE_HIP_OK;
}

int HitStage::Count(BatchIO& io, uint64_t hitCap, uint64_t n)
{
	cap = onDevice ? hitCap : std::min<uint64_t>(hitCap, n);   // a host call stages no more
	return io.Result(onDevice ? outCount : &count, 1, 1, &dCount);
}

int HitStage::Back()
{
	if (onDevice)
		return PIRE_HIP_OK;
	*outCount = count;
	const uint64_t written = std::min<uint64_t>(count, cap);
	hipError_t e = hipSuccess;
	for (uint32_t k = 0; k < nLists && written && e == hipSuccess; ++k)
		e = hipMemcpy(lists[k].host, lists[k].dev, size_t(written) * lists[k].width, hipMemcpyDeviceToHost);
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, backLabel);
}

int LaunchSelect(const SelectDevice& image, uint32_t states, uint32_t words, const uint32_t* stateIdx, uint64_t n,
                 const uint64_t* want, uint64_t* outMasks, uint64_t* outHits, uint64_t* outHitMasks, uint64_t hitCap,
                 uint64_t* outHitCount, hipStream_t stream)
{
	TilePass t(stream);
	const int rc = t.Front("pire_hip_select", "hipMallocAsync(select scratch)", n, outHitCount);
	if (rc || !t.s.tiles)
		return rc;
	SelectPass p;
	p.masks = image.masks;
	p.fin = image.fin;
	p.states = states;
	p.words = words;
	p.stateIdx = stateIdx;
	p.n = n;
	p.want = want;
	p.outMasks = outMasks;
	p.store16 = outMasks && words % 2 == 0 && reinterpret_cast<uintptr_t>(outMasks) % 16 == 0;
	p.outHits = outHits;
	p.outHitMasks = outHitMasks;
	// The LDS form reads states * 8 bytes per BLOCK to save 8 bytes per STRING: only where a block of the small grid
	// walks at least twice as many strings as the table has states
	const uint32_t ldsGrid = std::min(t.s.tiles, kSelLdsBlocks);
	const uint64_t ldsStrings = uint64_t((t.s.tiles + ldsGrid - 1) / ldsGrid) * kBlockThreads;
	const bool lds = words == 1 && (want || outMasks) && states <= kSelLdsStates && ldsStrings >= 2ull * states;
	if (lds) {
		const hipError_t e = SetDynamicLds(reinterpret_cast<const void*>(SelectClassifyKernel<true>), kSelLdsStates * 8);
		if (e != hipSuccess)
			return HipFail(e, "hipFuncSetAttribute(LDS)");
		hipLaunchKernelGGL(SelectClassifyKernel<true>, dim3(ldsGrid), dim3(kBlockThreads), size_t(states) * 8, stream, p, t.s);
	} else {
		hipLaunchKernelGGL(SelectClassifyKernel<false>, t.Grid(), dim3(kBlockThreads), 0, stream, p, t.s);
	}
	return t.Tail(p, outHits ? hitCap : 0, outHitCount, "select launch");
}

}  // namespace pirehip
