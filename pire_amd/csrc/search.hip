// Where the leftmost-longest match of a regexp lies inside a string (pire_hip_search): two reference searches, one launch.
//
//   t = LongestSuffix(R, string)                 R: the scanner of Fsm::Reverse() of `re` followed by anything   run.h:313-341
//   b = len - t                                  the leftmost position a match starts at
//   h = LongestPrefix(F, string from b)          F: the scanner of `re` (ShortestPrefix where asked for)         run.h:277-311
//   found = t >= 0 && h >= 0,  begin = b,  end = b + h                                        (include/pire_hip.h has the formulas)
//
// One string per lane, both legs in the same launch: a lane walks its string backwards through R (exact.hip's suffix walk,
// SuffixWalk), then forwards from where that walk says the match starts through F (exact.hip's prefix walk, PrefixWalk; the
// start of that leg has any alignment, which walk.h's block feeder takes).  Both tables' dense images sit in the block's LDS
// next to each other, R's first.  The backward leg reads every byte of the string from memory; the forward leg reads the
// blocks of the match again, which the lane has just had in its hands (cache hits).
//
// Plain HIP with compiler-placed waits: nothing here keeps data on its way in registers.

#include "device_common.h"
#include "walk.h"

namespace pirehip {

struct SearchParams {
	ScanParams rev, fwd;       // rev.startPerm: Initialize() (+ Step(EndMark) with THROUGH_END); fwd.startPerm: Initialize()
	uint32_t fwdStartBegin;    // F's Initialize() + Step(BeginMark): the forward leg's start where it starts at byte 0 (THROUGH_BEGIN)
	uint32_t longest, throughBegin, throughEnd;
	long long* outBegin;
	long long* outEnd;
};

__global__ __launch_bounds__(1024) void SearchKernel(SearchParams q)
{
	const ScanParams& pr = q.rev;
	const ScanParams& pf = q.fwd;
	extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
	const LdsLayout LR = MakeLayout(pr.hot, 0, kRotPitch, 0);
	const LdsLayout LF = MakeLayout(pf.hot, 0, kRotPitch, 0);
	uint8_t* ldsF = lds + LR.total;   // (a layout's total is a multiple of 16)
	LoadTableToLds(pr, lds, LR);
	LoadTableToLds(pf, ldsF, LF);
	const uint64_t n = pr.n;
	for (uint64_t s = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < n; s += uint64_t(gridDim.x) * blockDim.x) {
		const uint64_t b = pr.offsets[s];
		const uint64_t e1 = pr.offsets[s + 1];
		const uint64_t e = e1 >= b ? e1 : b;   // offsets that decrease: an empty string
		const uint64_t len = e - b;
		const uint64_t lo = reinterpret_cast<uint64_t>(pr.text) + b;
		const long long t = SuffixWalk(pr, lds, LR, lo, lo + len, 1u, q.throughBegin);
		long long begin = -1, end = -1;
		if (t >= 0) {
			const uint64_t from = len - uint64_t(t);   // t <= len: the walk counts the bytes it took
			const uint32_t st = q.throughBegin && from == 0 ? q.fwdStartBegin : pf.startPerm;
			const long long h = PrefixWalk(pf, ldsF, LF, pr.text + b + from, uint64_t(t), st, q.longest, q.throughEnd);
			if (h >= 0) {
				begin = (long long)from;
				end = (long long)from + h;
			}
		}
		q.outBegin[s] = begin;
		q.outEnd[s] = end;
	}
}

int LaunchSearch(const ScanParams& rev, const ScanParams& fwd, uint32_t fwdStartBegin, uint32_t opts, long long* outBegin,
                 long long* outEnd, hipStream_t stream)
{
	if (rev.n == 0)
		return PIRE_HIP_OK;
	SearchParams q;
	q.rev = rev;
	q.fwd = fwd;
	q.rev.compact = q.fwd.compact = 0;   // the dense rows only: no room for the warm rows of two tables
	q.fwd.n = rev.n;
	q.fwd.text = rev.text;
	q.fwd.offsets = rev.offsets;
	q.fwdStartBegin = fwdStartBegin;
	q.longest = (opts & PIRE_HIP_SEARCH_SHORTEST) ? 0 : 1;
	q.throughBegin = (opts & PIRE_HIP_SEARCH_THROUGH_BEGIN) ? 1 : 0;
	q.throughEnd = (opts & PIRE_HIP_SEARCH_THROUGH_END) ? 1 : 0;
	q.outBegin = outBegin;
	q.outEnd = outEnd;
	int cus = 0, dev = 0;
	if (int rc = DeviceCUs(&cus, &dev))
		return rc;
	const uint32_t ldsBytes = MakeLayout(rev.hot, 0, kRotPitch, 0).total + MakeLayout(fwd.hot, 0, kRotPitch, 0).total;
	int limit = 0;
	hipError_t e = hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
	if (e != hipSuccess)
		return HipFail(e, "hipDeviceGetAttribute(LDS per block)");
	if (ldsBytes > uint32_t(limit)) {   // (two tables of 255 dense rows take 137 312 bytes: not on a device with 160 KiB)
		SetError("pire_hip_search: the two tables' dense rows take " + std::to_string(ldsBytes) + " bytes of LDS, the device has " +
		         std::to_string(limit) + " per block");
		return PIRE_HIP_EUNSUPPORTED;
	}
	e = SetDynamicLds(reinterpret_cast<const void*>(SearchKernel), ldsBytes);
	if (e != hipSuccess)
		return HipFail(e, "hipFuncSetAttribute(LDS)");
	const unsigned threads = 1024;
	const unsigned blocks = unsigned(std::max<uint64_t>(1, std::min<uint64_t>((rev.n + threads - 1) / threads, uint64_t(cus) * 2)));
	hipLaunchKernelGGL(SearchKernel, dim3(blocks), dim3(threads), ldsBytes, stream, q);
	e = hipGetLastError();
	if (e != hipSuccess)
		return HipFail(e, "search kernel launch");
	return PIRE_HIP_OK;
}

}  // namespace pirehip
