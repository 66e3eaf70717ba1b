// Labelled matches and tokens (pire_hip_lex): which regexps of a glued Scanner accept each match -- Scanner::Glue followed by
// AcceptedRegexps, per match instead of per string.
//
// Search mode is search_all.hip's loop over R and F (match_loop.h: the same marks, the same MatchLoop), so spans, owners and
// rows are that call's.  Token mode needs no R:
//
//   p = 0
//   while p < len:
//       h = LongestPrefix(F, string from p)            (ShortestPrefix where asked for)                    run.h:277-311
//       h > 0: an entry [p, p + h) with its mask, p += h        else: byte p is a gap byte, p += 1
//   a maximal run of gap bytes is one entry with mask 0         (include/pire_hip.h has the formulas)
//
// The mask of an entry: F's state q after its h bytes -- LabelledPrefixWalk below is PrefixWalk (device_common.h) that also says
// which state set the length --, acceptMaskPerm[q] where Final(q), OR acceptMaskPerm[Step(q, EndMark)] where the walk took
// the EndMark at the string's end and that state is Final.  One or two 8-byte loads per entry, whatever rows the states have.
//
// Four launches on the caller's stream, one string per lane, 1 024-thread blocks, tables in LDS as search_all.hip has them:
//   count   search mode: the marks of the backward walk through R, then the forward loop; token mode: the loop above.
//           counts[i]; where label counts are asked for, every entry's label (its lowest bit; R for a gap) is tallied in the
//           block's LDS -- 64-bit integer adds, so the order does not matter --, and the block writes its R + 1 tallies out.
//   rows    search_all.hip's two scan kernels over the counts (LaunchSearchAllRows).
//   fill    block 0 sums the blocks' tallies into out_label_counts; the loop again into owners, spans and masks below the
//           capacity.  Gaps are coalesced inside the loop, so both passes number the entries alike.
// No global atomics, no scratch clearing: every word read was written in this call.  Plain HIP with compiler-placed waits.

#include "device_common.h"
#include "walk.h"
#include "compact.h"
#include "match_loop.h"

namespace pirehip {

namespace {

struct LexParams {
	SearchAllParams a;         // token mode: a.rev is a.fwd (the batch: n, text, offsets), no marks
	uint64_t* outMasks;        // nullable
	uint64_t* tallies;         // [blocks][regexps + 1], null where no label counts are asked for
	uint64_t* outLabelCounts;  // nullable
	uint32_t labels;           // regexps + 1
	uint32_t blocks;           // of the count launch
};

constexpr uint32_t kMaxLabels = 65;   // 64 regexps and the gaps

// PrefixWalk (device_common.h: LongestPrefix / ShortestPrefix, run.h:277-311) for one lane, which also answers the accept mask
// of the prefix it reports (*mask, where the length is > 0): of the state after its bytes where that state is Final, OR of the
// state behind the EndMark where that one set or confirmed a length that is the whole text.
__device__ __forceinline__ long long LabelledPrefixWalk(const ScanParams& p, const uint8_t* lds, const LdsLayout& L, const uint8_t* text,
                                                        uint64_t len, uint32_t st, uint32_t longest, uint32_t throughEnd, uint64_t* mask)
{
	long long pos = -1;
	uint32_t at = st;   // the state that set pos
	bool stop = false;
	uint32_t f = StateFlags(p, lds, L, st);
	if (f & kFinal) {
		pos = 0;
		stop = !longest;
	}
	const bool foundAtStart = stop;
	if (!stop) {
		uint64_t i = 0;
		auto step = [&](uint32_t byte) {
			st = SlowStep(p, lds, L, st, byte);
			f = StateFlags(p, lds, L, st);
			++i;
			if (f & kFinal) {
				pos = (long long)i;
				at = st;
				if (!longest)
					stop = true;
			}
			if (f & kDead)
				stop = true;
			return !stop;
		};
		// whole blocks through the dense rows alone where neither a Dead nor a Final state is among the 16 reached: nothing to record
		WalkBlocks(text, text + len, [&](walk_u32x4 v, uint32_t skip, uint32_t count) {
			if (st < p.hot) {
				uint32_t h = st;
				const uint32_t mx = count == 16 ? DenseChunk(lds, L, v, h) : DenseBytes(lds, L, v, skip, count, h);
				if (mx < p.hotDeadLo) {
					st = h;
					i += count;
					return true;
				}
			}
			return BlockBytes(v, skip, count, step);
		});
	}
	bool byBytes = pos > 0, byEnd = false;
	uint32_t end = 0;
	if (throughEnd && !foundAtStart) {
		end = p.nextPerm[size_t(st) * p.letters + p.endCls];
		if (StateFlags(p, lds, L, end) & kFinal) {
			if (longest || pos < 0) {
				byBytes = byBytes && pos == (long long)len;   // an earlier Final state no longer sets the length
				pos = (long long)len;
			}
			byEnd = pos == (long long)len;
		}
	}
	if (pos > 0)
		*mask = (byBytes ? p.acceptMaskPerm[at] : 0) | (byEnd ? p.acceptMaskPerm[end] : 0);
	return pos;
}

// The label an entry is counted under: its lowest regexp (lex's first-rule-wins), `gaps` for a gap
__device__ __forceinline__ uint32_t LabelOf(uint64_t mask, uint32_t gaps)
{
	return mask ? uint32_t(__builtin_ctzll(mask)) : gaps;
}

// The entries of string s (text + b, len bytes > 0): emit(k, begin, end, mask) for entry k; returns their number, `limit` at most
template <bool kTokens, class Emit>
__device__ __forceinline__ uint64_t LexLoop(const SearchAllParams& q, const uint8_t* ldsF, const LdsLayout& LF, uint64_t s, uint64_t b,
                                            uint64_t len, uint64_t limit, Emit&& emit)
{
	uint64_t mask = 0;
	auto walk = [&](const uint8_t* text, uint64_t bytes, uint32_t st) {
		return LabelledPrefixWalk(q.fwd, ldsF, LF, text, bytes, st, q.longest, q.throughEnd, &mask);
	};
	if (!kTokens)
		return MatchLoop(q, s, b, len, limit, walk, [&](uint64_t k, uint64_t begin, uint64_t end) { emit(k, begin, end, mask); });
	const uint8_t* str = q.fwd.text + b;
	uint64_t p = 0, k = 0, gap = 0;
	bool open = false;   // a gap run [gap, p) waits for its end
	while (p < len && k < limit) {
		const long long h = walk(str + p, len - p, q.throughBegin && p == 0 ? q.fwdStartBegin : q.fwd.startPerm);
		if (h > 0) {
			if (open) {
				emit(k, gap, p, uint64_t(0));
				++k;
				open = false;
				if (k == limit)
					break;
			}
			emit(k, p, p + uint64_t(h), mask);
			++k;
			p += uint64_t(h);
		} else {
			if (!open) {
				open = true;
				gap = p;
			}
			++p;
		}
	}
	if (open && k < limit) {
		emit(k, gap, len, uint64_t(0));
		++k;
	}
	return k;
}

template <bool kTokens>
__global__ __launch_bounds__(1024) void LexCountKernel(LexParams lp)
{
	const SearchAllParams& q = lp.a;
	const ScanParams& pr = q.rev;
	const ScanParams& pf = q.fwd;
	extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
	__shared__ unsigned long long tally[kMaxLabels];
	const LdsLayout LR = MakeLayout(pr.hot, 0, kRotPitch, 0);
	const LdsLayout LF = MakeLayout(pf.hot, 0, kRotPitch, 0);
	uint8_t* ldsF = kTokens ? lds : lds + LR.total;   // (a layout's total is a multiple of 16)
	if (threadIdx.x < kMaxLabels)
		tally[threadIdx.x] = 0;
	if (!kTokens)
		LoadTableToLds(pr, lds, LR);
	LoadTableToLds(pf, ldsF, LF);   // (ends with a barrier: the tallies are zero for everyone)
	const uint64_t n = pf.n;
	const uint32_t gaps = lp.labels - 1;
	for (uint64_t s = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < n; s += uint64_t(gridDim.x) * blockDim.x) {
		uint64_t b, len;
		StringOf(q, s, &b, &len);
		uint64_t count = 0;
		if (len) {
			if (!kTokens) {
				const uint64_t lo = reinterpret_cast<uint64_t>(pr.text) + b;
				MarkWalk(q, lds, LR, s, lo, lo + len);
			}
			count = LexLoop<kTokens>(q, ldsF, LF, s, b, len, ~uint64_t(0), [&](uint64_t, uint64_t, uint64_t, uint64_t mask) {
				if (lp.tallies)
					atomicAdd(&tally[LabelOf(mask, gaps)], 1ull);   // LDS, integers: any order gives the same sums
			});
		}
		q.counts[s] = count;
	}
	if (lp.tallies) {
		__syncthreads();
		if (threadIdx.x < lp.labels)
			lp.tallies[size_t(blockIdx.x) * lp.labels + threadIdx.x] = tally[threadIdx.x];
	}
}

// Block 0: the label counts from the blocks' tallies.  lists != 0: the loop again, into the lists.  rows[i] becomes the entries
// in front of string i in the batch.
template <bool kTokens>
__global__ __launch_bounds__(1024) void LexFillKernel(LexParams lp, uint32_t lists)
{
	const SearchAllParams& q = lp.a;
	const ScanParams& pf = q.fwd;
	extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
	const LdsLayout LF = MakeLayout(pf.hot, 0, kRotPitch, 0);
	if (lp.outLabelCounts && blockIdx.x == 0 && threadIdx.x < lp.labels) {
		uint64_t sum = 0;
		for (uint32_t blk = 0; blk < lp.blocks; ++blk)
			sum += lp.tallies[size_t(blk) * lp.labels + threadIdx.x];
		lp.outLabelCounts[threadIdx.x] = sum;
	}
	if (lists)
		LoadTableToLds(pf, lds, LF);
	const uint64_t n = pf.n;
	for (uint64_t s = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < n; s += uint64_t(gridDim.x) * blockDim.x) {
		const uint64_t row = q.rows[s] + q.tileSums[s / kBlockThreads];
		q.rows[s] = row;
		if (!lists || row >= q.cap)
			continue;
		const uint64_t count = q.counts[s];
		if (!count)
			continue;
		const uint64_t room = q.cap - row;
		uint64_t b, len;
		StringOf(q, s, &b, &len);
		const uint64_t base = b + q.shift * s;
		LexLoop<kTokens>(q, lds, LF, s, b, len, count < room ? count : room, [&](uint64_t k, uint64_t begin, uint64_t end, uint64_t mask) {
			if (q.outOwners)
				q.outOwners[row + k] = s;
			if (q.outSpans) {
				q.outSpans[2 * (row + k)] = base + begin;
				q.outSpans[2 * (row + k) + 1] = base + end;
			}
			if (lp.outMasks)
				lp.outMasks[row + k] = mask;
		});
	}
}

}  // namespace

int LaunchLex(const ScanParams& rev, const ScanParams& fwd, uint32_t fwdStartBegin, uint32_t opts, uint64_t textBytes, uint64_t shift,
              uint64_t* outRows, uint64_t* outOwners, uint64_t* outSpans, uint64_t* outMasks, uint64_t cap, uint64_t* outCount,
              uint64_t* outLabelCounts, hipStream_t stream)
{
	const bool tokens = (opts & PIRE_HIP_LEX_TOKENS) != 0;
	const uint64_t n = tokens ? fwd.n : rev.n;
	const uint32_t labels = fwd.regexps + 1;
	if (n == 0) {
		hipError_t e = hipMemsetAsync(outCount, 0, 8, stream);
		if (e == hipSuccess && outRows)
			e = hipMemsetAsync(outRows, 0, 8, stream);
		if (e == hipSuccess && outLabelCounts)
			e = hipMemsetAsync(outLabelCounts, 0, size_t(labels) * 8, stream);
		return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemsetAsync(entry count)");
	}
	if (!fwd.acceptMaskPerm || labels > kMaxLabels) {
		SetError("pire_hip_lex: fwd has no accept masks (more than 64 regexps)");
		return PIRE_HIP_EUNSUPPORTED;
	}
	LexParams lp;
	SearchAllParams& q = lp.a;
	q.fwd = fwd;
	q.fwd.compact = 0;   // the dense rows only, as search_all.hip
	if (tokens) {
		q.rev = q.fwd;   // the batch; its table is not read
	} else {
		q.rev = rev;
		q.rev.compact = 0;
		q.fwd.n = n;
		q.fwd.text = rev.text;
		q.fwd.offsets = rev.offsets;
	}
	q.fwdStartBegin = fwdStartBegin;
	q.longest = (opts & PIRE_HIP_LEX_SHORTEST) ? 0 : 1;
	q.throughBegin = (opts & PIRE_HIP_LEX_THROUGH_BEGIN) ? 1 : 0;
	q.throughEnd = (opts & PIRE_HIP_LEX_THROUGH_END) ? 1 : 0;
	q.textBytes = textBytes;
	q.shift = shift;
	q.outOwners = cap ? outOwners : nullptr;
	q.outSpans = cap ? outSpans : nullptr;
	lp.outMasks = cap ? outMasks : nullptr;
	q.cap = cap;
	q.outCount = outCount;
	q.marks = nullptr;
	lp.outLabelCounts = outLabelCounts;
	lp.labels = labels;
	int cus = 0, dev = 0;
	if (int rc = DeviceCUs(&cus, &dev))
		return rc;
	const uint32_t ldsF = MakeLayout(fwd.hot, 0, kRotPitch, 0).total;
	const uint32_t ldsBytes = (tokens ? 0 : MakeLayout(rev.hot, 0, kRotPitch, 0).total) + ldsF;
	int limit = 0;
	hipError_t e = hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
	if (e != hipSuccess)
		return HipFail(e, "hipDeviceGetAttribute(LDS per block)");
	if (ldsBytes + kMaxLabels * 8 > uint32_t(limit)) {
		SetError(std::string("pire_hip_lex: the dense rows of ") + (tokens ? "fwd" : "the two tables") + " and the label tallies take " +
		         std::to_string(ldsBytes + kMaxLabels * 8) + " bytes of LDS, the device has " + std::to_string(limit) + " per block");
		return PIRE_HIP_EUNSUPPORTED;
	}
	// one block of scratch: counts[n], tile sums, rows[n + 1] where the caller has no array for them, the blocks' tallies, the marks
	const uint32_t tiles = uint32_t((n + kBlockThreads - 1) / kBlockThreads);
	const unsigned threads = kBlockThreads;
	const unsigned blocks = unsigned(std::max<uint64_t>(1, std::min<uint64_t>(tiles, uint64_t(cus) * 2)));
	lp.blocks = blocks;
	const size_t markWords = tokens ? 0 : size_t(textBytes / 16) + size_t(n) + 2;
	const size_t tallyWords = outLabelCounts ? size_t(blocks) * labels : 0;
	const size_t words64 = size_t(n) + tiles + (outRows ? 0 : size_t(n) + 1) + tallyWords;
	StreamScratch scratch(stream);
	if (int rc = scratch.Alloc(words64 * 8 + markWords * 2, "hipMallocAsync(lex scratch)"))
		return rc;
	q.counts = scratch.as<uint64_t>();
	q.tileSums = q.counts + n;
	q.rows = outRows ? outRows : q.tileSums + tiles;
	lp.tallies = outLabelCounts ? scratch.as<uint64_t>() + (words64 - tallyWords) : nullptr;
	if (!tokens)
		q.marks = reinterpret_cast<uint16_t*>(scratch.as<uint64_t>() + words64);
	if (int rc = tokens ? Launch(LexCountKernel<true>, blocks, threads, ldsBytes, stream, "lex count launch", lp)
	                    : Launch(LexCountKernel<false>, blocks, threads, ldsBytes, stream, "lex marks launch", lp))
		return rc;
	if (int rc = LaunchSearchAllRows(q, tiles, stream))
		return rc;
	const uint32_t lists = q.outOwners || q.outSpans || lp.outMasks ? 1 : 0;
	if (!lists && !outRows && !outLabelCounts)
		return PIRE_HIP_OK;   // the count alone
	return tokens ? Launch(LexFillKernel<true>, blocks, threads, lists ? ldsF : 0, stream, "lex fill launch", lp, lists)
	              : Launch(LexFillKernel<false>, blocks, threads, lists ? ldsF : 0, stream, "lex fill launch", lp, lists);
}

}  // namespace pirehip
