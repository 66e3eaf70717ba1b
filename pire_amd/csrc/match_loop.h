// What search_all.hip and lex.hip share: the parameters of the list forms of the search, where a string lies, the mark words of
// the backward pass and the forward loop over them.  The row scan (SearchAllTileKernel, SearchAllSumKernel) stays in
// search_all.hip; lex.hip enqueues it through LaunchSearchAllRows.
#pragma once

#include "device_common.h"

namespace pirehip {

struct SearchAllParams {
	ScanParams rev, fwd;       // as SearchParams': rev.startPerm Initialize() (+ Step(EndMark)), fwd.startPerm Initialize()
	uint32_t fwdStartBegin;    // F's Initialize() + Step(BeginMark)
	uint32_t longest, throughBegin, throughEnd;
	uint64_t textBytes;        // offsets beyond it are clamped to it
	uint64_t shift;            // string i lies shift * i bytes further into the buffer the spans are counted in
	uint16_t* marks;           // [textBytes / 16 + n + 2]
	uint64_t* counts;          // [n] matches per string
	uint64_t* tileSums;        // [tiles]; after the scan: matches in front of the tile
	uint64_t* rows;            // [n + 1]; between the scans: matches in front of the string inside its tile
	uint64_t* outOwners;       // nullable
	uint64_t* outSpans;        // nullable
	uint64_t cap;
	uint64_t* outCount;
};

// search_all.hip: the exclusive 64-bit scan of q.counts[q.rev.n] on `stream`, two launches: q.rows[i] = the entries in front of
// string i inside its tile of 1 024, q.tileSums[tile] = the entries in front of the tile, q.rows[n] = *q.outCount = the total
int LaunchSearchAllRows(const SearchAllParams& q, uint32_t tiles, hipStream_t stream);

#if defined(__HIPCC__)

// String s of the batch: where it starts in the text and how long it is, both clamped to the text
__device__ __forceinline__ void StringOf(const SearchAllParams& q, uint64_t s, uint64_t* begin, uint64_t* len)
{
	const uint64_t o0 = q.rev.offsets[s], o1 = q.rev.offsets[s + 1];
	const uint64_t b = o0 < q.textBytes ? o0 : q.textBytes;
	const uint64_t e = o1 < q.textBytes ? o1 : q.textBytes;
	*begin = b;
	*len = e >= b ? e - b : 0;   // offsets that decrease: an empty string
}

// The word of the block at address `block` (a multiple of 16) of string s
__device__ __forceinline__ uint64_t MarkIndex(const SearchAllParams& q, uint64_t block, uint64_t s)
{
	return (block >> 4) - (reinterpret_cast<uint64_t>(q.rev.text) >> 4) + s;
}

// The backward walk of string s at addresses [lo, top) through R: LongestSuffix's loop (run.h:326-340), which writes the
// marks of every position instead of remembering the lowest one.
__device__ __forceinline__ void MarkWalk(const SearchAllParams& q, const uint8_t* lds, const LdsLayout& L, uint64_t s, uint64_t lo, uint64_t top)
{
	const ScanParams& p = q.rev;
	uint64_t cur = top;   // one past the next byte to take
	uint32_t st = p.startPerm;
	bool dead = (StateFlags(p, lds, L, st) & kDead) != 0;
	while (cur > lo) {
		const uint64_t block = (cur - 1) & ~uint64_t(15);
		uint32_t k = uint32_t(cur - 1 - block);                          // index of the next byte inside the block
		const uint32_t kLow = block >= lo ? 0u : uint32_t(lo - block);   // first index that belongs to the string
		uint32_t word = 0;
		if (dead) {
			cur = block + kLow;   // below a Dead state: no marks, the text is not read
		} else {
			u32x4 v = *reinterpret_cast<const u32x4*>(block);
			bool taken = false;
			// a whole block from a state with a dense row: neither a Dead nor a Final state among the sixteen reached (the
			// rows are ordered plain, Dead, Final) -> no marks in it, take the state
			if (k == 15 && kLow == 0 && st < p.hot) {
				uint32_t h = st, mx = 0;
#pragma unroll
				for (int w = 3; w >= 0; --w) {
					const uint32_t x = v[w];
#pragma unroll
					for (int b2 = 3; b2 >= 0; --b2) {
						h = lds[h * L.pitch + ((x >> (8 * b2)) & 0xFFu)];
						mx = mx > h ? mx : h;
					}
				}
				if (mx < p.hotDeadLo) {
					st = h;
					cur -= 16;
					taken = true;
				}
			}
			if (!taken) {
				// bring byte k to the top of the 128-bit value, then peel bytes off the top
				for (uint32_t sh = 15 - k; sh; --sh) {
					v.w = __builtin_amdgcn_alignbit(v.w, v.z, 24);
					v.z = __builtin_amdgcn_alignbit(v.z, v.y, 24);
					v.y = __builtin_amdgcn_alignbit(v.y, v.x, 24);
					v.x <<= 8;
				}
				for (;;) {
					st = SlowStep(p, lds, L, st, v.w >> 24);
					const uint32_t f = StateFlags(p, lds, L, st);
					--cur;
					if (f & kFinal)
						word |= 1u << k;   // the suffix from byte k of the block matches
					dead = (f & kDead) != 0;
					if (dead || k == kLow)
						break;
					--k;
					v.w = __builtin_amdgcn_alignbit(v.w, v.z, 24);
					v.z = __builtin_amdgcn_alignbit(v.z, v.y, 24);
					v.y = __builtin_amdgcn_alignbit(v.y, v.x, 24);
					v.x <<= 8;
				}
				if (dead)
					cur = block + kLow;   // the rest of the block has no marks either
			}
			if (cur == lo && !dead && q.throughBegin) {   // run.h:336-340, byte 0 only
				const uint32_t sb = p.nextPerm[size_t(st) * p.letters + p.beginCls];
				if (StateFlags(p, lds, L, sb) & kFinal)
					word |= 1u << kLow;
			}
		}
		q.marks[MarkIndex(q, block, s)] = uint16_t(word);
	}
}

// The forward loop of string s (text + b, len bytes) over its marks: emit(k, begin, end) for match k; returns their number.
// walk(text, len, start state): the forward leg, LongestPrefix / ShortestPrefix through F -- the length of the prefix, -1
// where the reference returns null.  `limit`: no more than that many (the fill pass: what the count pass counted).
template <class Walk, class Emit>
__device__ __forceinline__ uint64_t MatchLoop(const SearchAllParams& q, uint64_t s, uint64_t b, uint64_t len, uint64_t limit, Walk&& walk,
                                              Emit&& emit)
{
	const uint8_t* str = q.rev.text + b;
	const uint64_t lo = reinterpret_cast<uint64_t>(str);
	const uint64_t lastBlock = (lo + len - 1) & ~uint64_t(15);   // (len > 0 where it is used)
	uint64_t p = 0, k = 0;
	while (p < len && k < limit) {
		// the next mark at or behind p
		uint64_t block = (lo + p) & ~uint64_t(15);
		uint32_t word = q.marks[MarkIndex(q, block, s)] & (0xFFFFu << uint32_t((lo + p) & 15));
		while (!word && block < lastBlock) {
			block += 16;
			word = q.marks[MarkIndex(q, block, s)];
		}
		if (!word)
			break;
		const uint64_t at = block + uint32_t(__builtin_ctz(word));
		if (at < lo || at - lo >= len)   // (strings that overlap in the text: another lane's bits)
			break;
		const uint64_t from = at - lo;
		const long long h = walk(str + from, len - from, q.throughBegin && from == 0 ? q.fwdStartBegin : q.fwd.startPerm);
		if (h < 0)
			break;   // two tables that do not belong together
		if (h > 0) {
			emit(k, from, from + uint64_t(h));
			++k;
		}
		p = from + (h > 0 ? uint64_t(h) : 1u);   // one byte past an empty match
	}
	return k;
}

#endif  // __HIPCC__

}  // namespace pirehip
