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
// Both kernels and the launcher are tile_pass.h's, the staging of the count and the list is internal.h's HitStage; this
// unit keeps its predicate and what a selected lane writes (FinalPass).  Launches on the caller's stream, the shape of
// select.hip: no block waits for another block, no atomics (the same input gives the same bits).
// Plain HIP with compiler-placed waits: nothing here keeps data on its way in registers.  A flag is read with a byte load
// (a wave reads 64 consecutive bytes, a tile 1 KiB): `final` may have any alignment.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "tile_pass.h"

namespace pirehip {

namespace {

struct FinalPass {
	const uint8_t* fin;   // [n]
	uint32_t invert;      // PIRE_HIP_FINAL_SELECT_ZERO
	uint64_t* outHits;

	__device__ __forceinline__ bool Selected(uint64_t i) const { return (fin[i] != 0) != (invert != 0); }
	__device__ __forceinline__ void Write(uint64_t rank, uint64_t i) const { outHits[rank] = i; }
};

}  // namespace

int LaunchFinalSelect(const uint8_t* fin, uint64_t n, uint32_t mode, uint64_t* outHits, uint64_t hitCap, uint64_t* outHitCount,
                      hipStream_t stream)
{
	TilePass t(stream);
	const int rc = t.Front("pire_hip_final_select", "hipMallocAsync(final select scratch)", n, outHitCount);
	if (rc || !t.s.tiles)
		return rc;
	const FinalPass p = {fin, mode == PIRE_HIP_FINAL_SELECT_ZERO, outHits};
	t.Classify(p, n);
	return t.Tail(p, outHits ? hitCap : 0, outHitCount, "final select launch");
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
	if (list.onDevice)
		return LaunchFinalSelect(nullptr, 0, o.mode, nullptr, 0, o.outHitCount, stream);
	*o.outHitCount = 0;
	return PIRE_HIP_OK;
}

int FinalSelectStage::Results(BatchIO& io, uint64_t n)
{
	if (int rc = list.Count(io, o.hitCap, n))
		return rc;
	return list.List(io, o.outHits, 1, &dHits);
}

int FinalSelectStage::Launch(const uint8_t* fin, uint64_t n, hipStream_t stream)
{
	return LaunchFinalSelect(fin, n, o.mode, dHits, list.cap, list.dCount, stream);
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
