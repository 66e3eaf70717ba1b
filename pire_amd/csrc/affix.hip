// From prefix and suffix lengths to matched heads and tails on the device (pire_hip_affix_select): which strings matched, and
// where the matched text -- or what it leaves -- lies.
//
// pire_hip_prefix and pire_hip_suffix answer with one length per string.  What their caller wants is the TEXT: the header a
// line starts with, the extension it ends with, what is left once leading and trailing blanks are taken off -- a compacted,
// ascending list of byte ranges, the input form of pire_hip_gather_spans.  This unit turns the one into the other without
// leaving the device.  It takes no table and no text: it reads lengths and offsets, whoever wrote them (include/pire_hip.h
// has the formulas):
//
//   classify  one lane per string: head_len and tail_len where they are given -- 16 bytes, coalesced -> selected?  The
//             selected bits of a wave are one ballot word, kept in scratch; one count per tile of 1 024 strings.
//   scan      exclusive scan of the tile counts, one block; the total is the hit count (select.hip's kernel, LaunchTileScan).
//   scatter   rank of a selected string = tile offset + the popcounts of the waves in front + mbcnt of its own wave's
//             ballot word; the lane computes its span from offsets and lengths, clamped into the string.
//
// Both kernels and the launcher are tile_pass.h's, the staging of the count and the lists is internal.h's HitStage; this
// unit keeps its predicate and what a selected lane writes (AffixPass).  Three launches on the caller's stream, the shape
// of select.hip: no block waits for another block, no atomics (the same input gives the same bits).
// Plain HIP with compiler-placed waits: nothing here keeps data on its way in registers.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "tile_pass.h"

namespace pirehip {

namespace {

struct AffixPass {
	const uint64_t* offsets;
	const long long* headLen;   // nullable: no head was looked for
	const long long* tailLen;   // nullable: no tail was looked for
	uint32_t part;              // PIRE_HIP_AFFIX_HEAD / _TAIL / _REST
	uint64_t shift;             // string i lies shift * i bytes further into the buffer of the spans
	uint64_t* outHits;          // nullable
	uint64_t* outSpans;         // nullable

	__device__ __forceinline__ bool Selected(uint64_t i) const { return (!headLen || headLen[i] >= 0) && (!tailLen || tailLen[i] >= 0); }
	// (a selected bit: the lengths that are given are >= 0)
	__device__ __forceinline__ void Write(uint64_t rank, uint64_t i) const
	{
		if (outHits)
			outHits[rank] = i;
		if (outSpans) {
			const uint64_t o0 = offsets[i], o1 = offsets[i + 1];
			const uint64_t len = o1 >= o0 ? o1 - o0 : 0;   // (offsets that decrease: an empty string)
			const uint64_t h = headLen ? std::min<uint64_t>(uint64_t(headLen[i]), len) : 0;
			const uint64_t base = o0 + shift * i;
			uint64_t b, e;
			if (part == PIRE_HIP_AFFIX_HEAD) {
				b = 0, e = h;
			} else if (part == PIRE_HIP_AFFIX_TAIL) {
				b = len - std::min<uint64_t>(uint64_t(tailLen[i]), len), e = len;
			} else {   // REST: the tail gives way to the head where they overlap
				b = h, e = len - (tailLen ? std::min<uint64_t>(uint64_t(tailLen[i]), len - h) : 0);
			}
			outSpans[2 * rank] = base + b;
			outSpans[2 * rank + 1] = base + e;
		}
	}
};

}  // namespace

int LaunchAffixSelect(const uint64_t* offsets, uint64_t n, uint32_t part, const long long* headLen, const long long* tailLen,
                      uint64_t shift, uint64_t* outHits, uint64_t* outSpans, uint64_t hitCap, uint64_t* outHitCount, hipStream_t stream)
{
	TilePass t(stream);
	const int rc = t.Front("pire_hip_affix_select", "hipMallocAsync(affix select scratch)", n, outHitCount);
	if (rc || !t.s.tiles)
		return rc;
	const AffixPass p = {offsets, headLen, tailLen, part, shift, outHits, outSpans};
	t.Classify(p, n);
	return t.Tail(p, outHits || outSpans ? hitCap : 0, outHitCount, "affix select launch");
}

int AffixSelectArgsInvalid(const char* who, uint64_t n, bool haveOffsets, bool haveHead, bool haveTail, const AffixSelectOut& o, bool ownList)
{
	const char* what = o.part > PIRE_HIP_AFFIX_REST                    ? "unknown part"
	                   : !o.outHitCount                                ? "null out_hit_count"
	                   : n && !haveHead && !haveTail                   ? "n > 0 with null head_len and null tail_len"
	                   : o.part == PIRE_HIP_AFFIX_HEAD && !haveHead    ? "PIRE_HIP_AFFIX_HEAD without head_len"
	                   : o.part == PIRE_HIP_AFFIX_TAIL && !haveTail    ? "PIRE_HIP_AFFIX_TAIL without tail_len"
	                   : n && !haveOffsets                             ? "n > 0 with null offsets"
	                   : o.hitCap && !o.outHits && !o.outSpans && !ownList ? "hit_cap > 0 with null out_hits and null out_spans"
	                   : n >= (1ull << 32)                             ? "2^32 strings or more in one call"
	                                                                   : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

int AffixSelectStage::Empty(hipStream_t stream)
{
	if (list.onDevice)
		return LaunchAffixSelect(nullptr, 0, o.part, nullptr, nullptr, 0, nullptr, nullptr, 0, o.outHitCount, stream);
	*o.outHitCount = 0;
	return PIRE_HIP_OK;
}

int AffixSelectStage::Results(BatchIO& io, uint64_t n)
{
	int rc;
	if ((rc = list.Count(io, o.hitCap, n)) || (rc = list.List(io, o.outHits, 1, &dHits)))
		return rc;
	return list.List(io, o.outSpans, 2, &dSpans);
}

int AffixSelectStage::Launch(const uint64_t* offsets, uint64_t n, const int64_t* headLen, const int64_t* tailLen, hipStream_t stream)
{
	return LaunchAffixSelect(offsets, n, o.part, reinterpret_cast<const long long*>(headLen), reinterpret_cast<const long long*>(tailLen), 0,
	                         dHits, dSpans, list.cap, list.dCount, stream);
}

}  // namespace pirehip

using namespace pirehip;

extern "C" int pire_hip_affix_select(const uint64_t* offsets, uint64_t n, uint32_t part, uint32_t flags, const int64_t* head_len,
                                     const int64_t* tail_len, uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap,
                                     uint64_t* out_hit_count, void* streamPtr)
try {
	const AffixSelectOut o = {part, out_hits, out_spans, hit_cap, out_hit_count};
	if (int rc = AffixSelectArgsInvalid("pire_hip_affix_select", n, offsets != nullptr, head_len != nullptr, tail_len != nullptr, o))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	AffixSelectStage pass(o, onDevice);
	if (n == 0)
		return pass.Empty(stream);
	// host pointers: staged in, the three kernels, staged out -- the lists only as far as they were written.  (Offsets that
	// decrease are not refused here: the pass has a meaning for them, and reads no text through them.)
	BatchIO io(stream, onDevice);
	const uint64_t* dOffsets = nullptr;
	const int64_t *dHead = nullptr, *dTail = nullptr;
	int rc;
	if ((rc = io.In(offsets, size_t(n) + 1, &dOffsets)))
		return rc;
	if (head_len)
		if ((rc = io.In(head_len, size_t(n), &dHead)))
			return rc;
	if (tail_len)
		if ((rc = io.In(tail_len, size_t(n), &dTail)))
			return rc;
	if ((rc = pass.Results(io, n)) || (rc = io.Ready()))
		return rc;
	if ((rc = pass.Launch(dOffsets, n, dHead, dTail, stream)))
		return rc;
	if ((rc = io.Finish()))
		return rc;
	return pass.Back();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}
