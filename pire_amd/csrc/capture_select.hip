// From capture positions to captured substrings on the device (pire_hip_capture_select): which strings captured, and where.
//
// pire_hip_capture_run answers with two step counters per string.  What a caller of a capturing scanner wants is the
// captured TEXT of the strings that captured at all -- a compacted, ascending list of byte ranges, the input form of
// pire_hip_gather_spans.  This unit turns the one into the other without leaving the device, behind ANY of the capture
// kernels (it reads positions, offsets and Final flags, nothing else of a scan; include/pire_hip.h has the formulas):
//
//   classify  one lane per string: begin, end and, where asked for, final -- 17 bytes, coalesced -> selected?  The selected
//             bits of a wave are one ballot word, kept in scratch; one count per tile of 1 024 strings.
//   scan      exclusive scan of the tile counts, one block; the total is the hit count (select.hip's kernel, LaunchTileScan).
//   scatter   rank of a selected string = tile offset + the popcounts of the waves in front + mbcnt of its own wave's
//             ballot word; the lane computes its span again from offsets and positions, clamped into the string.
//
// Both kernels and the launcher are tile_pass.h's, the staging of the count and the lists is internal.h's HitStage; this
// unit keeps its predicate and what a selected lane writes (CapturePass).  Three launches on the caller's stream, the shape
// of select.hip: no block waits for another block, no atomics (the same input gives the same bits).  Plain HIP with
// compiler-placed waits: nothing here keeps data on its way in registers.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "tile_pass.h"

namespace pirehip {

namespace {

struct CapturePass {
	const uint64_t* offsets;
	const long long* begin;
	const long long* end;
	const uint8_t* fin;      // nullable: Final is not asked for
	long long beginMark;     // B: 1 where the BeginMark step was counted
	uint64_t shift;          // string i lies shift * i bytes further into the buffer of the spans
	uint64_t* outHits;       // nullable
	uint64_t* outSpans;      // nullable

	__device__ __forceinline__ bool Selected(uint64_t i) const { return begin[i] >= 0 && end[i] >= 0 && (!fin || fin[i] != 0); }
	// (a selected bit: begin >= 0 and end >= 0)
	__device__ __forceinline__ void Write(uint64_t rank, uint64_t i) const
	{
		if (outHits)
			outHits[rank] = i;
		if (outSpans) {
			const uint64_t o0 = offsets[i], o1 = offsets[i + 1];
			const uint64_t len = o1 >= o0 ? o1 - o0 : 0;   // (offsets that decrease: an empty string)
			// begin >= 0 and B <= 1: the differences cannot wrap
			const long long bb = begin[i] - beginMark, ee = end[i] - beginMark;
			const uint64_t b = bb < 0 ? 0 : std::min<uint64_t>(uint64_t(bb), len);
			const uint64_t e = ee < 0 ? b : std::min<uint64_t>(std::max<uint64_t>(uint64_t(ee), b), len);
			const uint64_t base = o0 + shift * i;
			outSpans[2 * rank] = base + b;
			outSpans[2 * rank + 1] = base + e;
		}
	}
};

}  // namespace

int LaunchCaptureSelect(const uint64_t* offsets, uint64_t n, bool beginMark, const long long* begin, const long long* end,
                        const uint8_t* fin, uint64_t shift, uint64_t* outHits, uint64_t* outSpans, uint64_t hitCap,
                        uint64_t* outHitCount, hipStream_t stream)
{
	TilePass t(stream);
	const int rc = t.Front("pire_hip_capture_select", "hipMallocAsync(capture select scratch)", n, outHitCount);
	if (rc || !t.s.tiles)
		return rc;
	const CapturePass p = {offsets, begin, end, fin, beginMark ? 1 : 0, shift, outHits, outSpans};
	t.Classify(p, n);
	return t.Tail(p, outHits || outSpans ? hitCap : 0, outHitCount, "capture select launch");
}

int CaptureSelectOutputsInvalid(const char* who, uint64_t n, int needFinal, bool haveFinal, bool haveList, uint64_t hitCap,
                                const void* outHitCount)
{
	const char* what = !outHitCount                          ? "null out_hit_count"
	                   : needFinal && !haveFinal             ? "need_final with null final"
	                   : hitCap && !haveList                 ? "hit_cap > 0 with null out_hits and null out_spans"
	                   : n >= (1ull << 32)                   ? "2^32 strings or more in one call"
	                                                         : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

}  // namespace pirehip

using namespace pirehip;

extern "C" int pire_hip_capture_select(const uint64_t* offsets, uint64_t n, uint32_t flags, const int64_t* begin, const int64_t* end,
                                       const uint8_t* fin, int need_final, uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap,
                                       uint64_t* out_hit_count, void* streamPtr)
try {
	const char* who = "pire_hip_capture_select";
	if (int rc = CaptureSelectOutputsInvalid(who, n, need_final, fin != nullptr, out_hits || out_spans, hit_cap, out_hit_count))
		return rc;
	if (n && (!offsets || !begin || !end)) {
		SetError(std::string(who) + ": n > 0 with null offsets, begin or end");
		return PIRE_HIP_EINVAL;
	}
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	const bool beginMark = (flags & PIRE_HIP_RUN_BEGIN) != 0;
	if (!need_final)
		fin = nullptr;
	if (onDevice)
		return LaunchCaptureSelect(offsets, n, beginMark, reinterpret_cast<const long long*>(begin), reinterpret_cast<const long long*>(end),
		                           fin, 0, out_hits, out_spans, hit_cap, out_hit_count, stream);
	if (n == 0) {
		*out_hit_count = 0;
		return PIRE_HIP_OK;
	}
	if (int rc = CheckOffsets(offsets, n))
		return rc;
	// host pointers: staged in, the three kernels, staged out -- the lists only as far as they were written
	BatchIO io(stream, false);
	const uint64_t* dOffsets = nullptr;
	const int64_t *dBegin = nullptr, *dEnd = nullptr;
	const uint8_t* dFin = nullptr;
	int rc;
	if ((rc = io.In(offsets, size_t(n) + 1, &dOffsets)) || (rc = io.In(begin, size_t(n), &dBegin)) || (rc = io.In(end, size_t(n), &dEnd)))
		return rc;
	if (fin)
		if ((rc = io.In(fin, size_t(n), &dFin)))
			return rc;
	HitStage list(false, out_hit_count, "hipMemcpy(hits)");
	uint64_t *dHits = nullptr, *dSpans = nullptr;
	if ((rc = list.Count(io, hit_cap, n)) || (rc = list.List(io, out_hits, 1, &dHits)) || (rc = list.List(io, out_spans, 2, &dSpans)) ||
	    (rc = io.Ready()))
		return rc;
	if ((rc = LaunchCaptureSelect(dOffsets, n, beginMark, reinterpret_cast<const long long*>(dBegin), reinterpret_cast<const long long*>(dEnd),
	                              dFin, 0, dHits, dSpans, list.cap, list.dCount, stream)))
		return rc;
	if ((rc = io.Finish()))
		return rc;
	return list.Back();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}
