// Internal structures of libpire_hip.so (not installed).  See DESIGN.md for the data layout.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <atomic>
#include <memory>
#include <mutex>
#include <optional>
#include <shared_mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/pire_hip.h"

namespace pirehip {

// pire/defs.h:59-73
enum : uint32_t {
	kEpsilon = 257,
	kBeginMark = 258,
	kEndMark = 259,
	kMaxCharUnaligned = 260,
	kMaxChar = 264,
};

enum : uint8_t {
	kFinal = 1,      // FinalFlag, multi.h:91
	kDead = 2,       // DeadFlag,  multi.h:92
	kAbsorbing = 4,  // ours: every transition of the row (all letter classes, marks included) is a self loop
};

constexpr uint32_t kMaxHotRows = 256;   // dense rows addressable by a u8 state id (255 hot + 1 trap)

// LDS carve-up shared by the scan kernels (single dynamic region, 16-byte aligned pieces).
struct LdsLayout {
	uint32_t pitch;        // bytes between dense rows: 260 = 65 dwords rotates row r by r banks, or 256
	uint32_t hotBytes;     // (hot+1)*pitch, rounded up to 16
	uint32_t flagsOff;     // 256 B of hot flags
	uint32_t cls8Off;      // 256 B: 2 * letter class of every byte (compact tier; 256-byte aligned when pitch == 256)
	uint32_t compactOff;   // compact tier: class-indexed u16 rows of the first `compact` states + the escape row
	uint32_t compactBytes;
	uint32_t clsOff;       // 264 u16 (generic kernel + slow step)
	uint32_t countsOff;    // (regexps+2) u32 block-local counters
	uint32_t histOff;      // 256 u32: sampled visits of hot ids (feeds pire_hip_table_adapt)
	uint32_t progOff;      // u32: tiles walked by the waves of the block (tiled kernel: keeps them in step)
	uint32_t total;
	uint32_t rot2;         // the dense rows' columns are in ROTATED byte order (column of byte b = rotl8(b, 2)): tiled kernel variant
};

// Column of input byte b in a dense row whose columns are rotated (LdsLayout::rot2): the LDS bank of a lookup is then
// b & 63 instead of (b >> 2) & 63 -- printable text spreads over all 64 banks instead of 24.
__host__ __device__ inline uint32_t RotColumn(uint32_t b) { return ((b << 2) | (b >> 6)) & 0xFFu; }

constexpr uint32_t kRotPitch = 260;
constexpr uint32_t kMaxLdsCountRegexps = 1024;
constexpr uint32_t kCheckSlot = 256;                     // visitHot[256]: failures seen by the checked kernel build
constexpr uint32_t kTrapSlot = 257;                      // visitHot[257]: sampled traps since the image was uploaded (device total)
constexpr uint32_t kWideTrapSlot = 258;                 // visitHot[258]: sampled chunks the WIDE walk left its rows in
constexpr uint32_t kVisitHotSlots = 260;
constexpr uint32_t kLdsTrapSlot = 257;                   // the same count inside a block: hist[257] in LDS (hist[256] = progress)
constexpr uint32_t kLdsPerBlock = 160 * 1024;            // gfx950: 160 KiB per CU, one block per CU may have it all
constexpr uint32_t kRaggedFinBytes = 256 * 16;           // ragged kernel: end-of-string records of the hot states
constexpr uint32_t kRaggedLdsExtra = kRaggedFinBytes + 32;

// The compact region sits right behind the dense rows so that its LDS addresses do not depend on the per-launch
// pieces (counters): the rows hold LDS addresses.
__host__ __device__ inline LdsLayout MakeLayout(uint32_t hot, uint32_t regexps, uint32_t pitch = kRotPitch,
                                                uint32_t compactBytes = 0)
{
	LdsLayout l;
	l.pitch = pitch;
	l.hotBytes = ((hot + 1) * pitch + 15) / 16 * 16;
	l.flagsOff = l.hotBytes;
	l.cls8Off = l.flagsOff + 256;
	l.compactOff = l.cls8Off + 256;
	l.compactBytes = (compactBytes + 15) / 16 * 16;
	l.clsOff = l.compactOff + l.compactBytes;
	l.countsOff = l.clsOff + 528;
	l.histOff = l.countsOff + ((regexps + 2) * 4 + 15) / 16 * 16;
	l.progOff = l.histOff + 1024;   // 16 B: the tiled kernel's block-wide progress counter
	l.total = l.progOff + 16;
	l.rot2 = 0;
	return l;
}

// Compact tier geometry: row = `letters` u16 entries + 1 u16 holding the row's own state id, padded to 4 bytes.
__host__ __device__ inline uint32_t CompactPitch(uint32_t letters) { return ((letters + 1) * 2 + 3) / 4 * 4; }

// How many states get a compact row next to everything else any kernel keeps in LDS (0 = tier off).
inline uint32_t CompactCapacity(uint32_t hot, uint32_t letters, uint32_t regexps, uint32_t states)
{
	if (letters > 127)
		return 0;   // the per-byte class table holds 2*class in a u8
	const uint32_t base = MakeLayout(hot, regexps <= kMaxLdsCountRegexps ? regexps : 0, 256u).total + kRaggedLdsExtra;
	if (base >= kLdsPerBlock)
		return 0;
	const uint32_t rows = (kLdsPerBlock - base) / CompactPitch(letters);
	if (rows < hot + 2 || states <= hot)
		return 0;   // no room beyond the hot states, or nothing beyond them
	return rows - 1 < states ? rows - 1 : states;
}

// ---- the wide walk (wide.hip, round 5) ---------------------------------------------------------------------------------
// Tables whose scans keep leaving the 255 dense rows take a walk of their own: NO dense rows, the whole LDS of the CU
// holds class-indexed u16 rows of the first `wide` states of the ranking (multi.h:169-192 as it stands: letter =
// m_letters[ch], state = row[letter]).  A row is
//     u16 next[letters]   device id of the target state; `wide` (the escape row's id) for targets without a row
//     u16 flags           kFinal | kDead | kAbsorbing of the state
// + 2 bytes where that makes a multiple of 8 (WidePitch); row `wide`, the escape row, leads to itself.  cls8 (2 * letter class of every byte
// value) sits at LDS address 0, so that the byte IS the address of its class.  Behind the rows: one u32 visit counter
// per row (what pire_hip_table_adapt() ranks from).
struct WideLayout {
	uint32_t pitch;      // bytes per row
	uint32_t rowsOff;    // 256
	uint32_t rows;       // states with a row + 1 (the last one is the escape row): wide + 1, zipped image: full + 1
	uint32_t full;       // zipped image (below): states with a row of their own; else == wide
	uint32_t hOff;       // zipped image: u32 header of every state of the tier and of the escape state (wide + 1 of them)
	uint32_t xOff;       // zipped image: 3 x u16 exception targets of every state WITHOUT a row of its own (wide - full of them)
	uint32_t imageEnd;   // end of what is copied from memory (rows [+ headers + exceptions]), 16-byte aligned
	uint32_t histOff;    // u32[rows]
	uint32_t countsOff;  // (regexps + 2) u32 block-local match counters
	uint32_t progOff;    // u32 progress counter of the block's waves + u32 trap samples
	uint32_t total;
};

// (a number of HALFWORDS per row that is not a multiple of four -- an odd number of dwords, or of halfwords: rows then start
// in every LDS bank in turn, in the second case at either half of its dword -- with 18
// dwords, 34 letters, the lanes of a wave that read the same letter's entry of different rows would share 16 of the 32
// banks.  Round 5 first padded to an odd number of DWORDS, 76 bytes for 34 letters; 70 do the same for the banks and
// leave room for 8 % more rows.)
__host__ __device__ inline uint32_t WidePitch(uint32_t letters)
{
	const uint32_t halfwords = letters + 1;   // the row's entries + its flags
	return (halfwords % 4 ? halfwords : halfwords + 1) * 2;
}

// ---- the zipped image (round 6) ----------------------------------------------------------------------------------------
// A dictionary automaton's rows are nearly all "the row of a shallower state, except for the one or two letters that
// continue a word" (the failure-link structure of the reference's determinised `word1|word2|...`, samples/blacklist/
// blacklist.cpp:65-76) -- a 70-byte row per state keeps 2 207 states of dict_10k's 30 202 in a CU's LDS, and from 3 % of the
// steps outside them on the walk is bound by the L2's request rate.  The zipped image keeps a full row only
// for `full` states (<= 1 023) and, for every other state of the tier, 10 bytes:
//     u32 header    bits 22..31  index of the full row this state's row is equal to except in <= 3 letters
//                   bits 1..7 / 8..14 / 15..21  those letter classes (127 = none)  [= 2 * class * 0x4081: ONE multiply of the
//                   byte's doubled class compares all three]
//     u16 target[3] where they lead
// States with a row of their own have a header too (base = themselves, no letters): the step is the same code for every
// lane --  h = header[st];  entry address = letter matches one of h's ? &target[st][k] : &row[h.base][letter];  st = u16 at it.
// Two dependent LDS reads per byte instead of one, 3 LDS instructions instead of 2: slower while the working set fits
// the plain rows, 4 x the states in LDS when it does not.  Device numbering: full states first, then the rest of the tier.
constexpr uint32_t kZipMaxFull = 1022;      // + the escape row: 10 bits of base
constexpr uint32_t kZipNoLetter = 127;
constexpr uint32_t kZipExceptions = 3;
constexpr uint32_t kZipMulC2 = 0x4081u;     // (2 * class) * 0x4081 = class at bits 1, 8, 15

__host__ __device__ inline WideLayout MakeWideLayout(uint32_t wide, uint32_t letters, uint32_t regexps, uint32_t zipFull = 0)
{
	WideLayout w;
	w.pitch = WidePitch(letters);
	w.rowsOff = 256;
	w.full = zipFull ? zipFull : wide;
	w.rows = w.full + 1;
	w.hOff = (w.rowsOff + w.rows * w.pitch + 3) / 4 * 4;
	w.xOff = w.hOff + (zipFull ? (wide + 1) * 4 : 0);
	w.imageEnd = (w.xOff + (zipFull ? (wide - zipFull) * 2 * kZipExceptions : 0) + 15) / 16 * 16;
	w.histOff = w.imageEnd;
	w.countsOff = (w.histOff + w.rows * 4 + 15) / 16 * 16;
	w.progOff = w.countsOff + ((regexps + 2) * 4 + 15) / 16 * 16;
	w.total = w.progOff + 16;
	return w;
}

// How many states get a wide row (0: the wide walk is not for this table).
inline uint32_t WideCapacity(uint32_t letters, uint32_t regexps, uint32_t states)
{
	if (letters > 127 || states < 2)
		return 0;   // cls8 holds 2 * class in a u8
	const uint32_t fixed = MakeWideLayout(0, letters, regexps <= kMaxLdsCountRegexps ? regexps : 0).total + 64;
	if (fixed >= kLdsPerBlock)
		return 0;
	const uint32_t rows = (kLdsPerBlock - fixed) / (WidePitch(letters) + 4);
	if (rows < 2)
		return 0;
	return rows - 1 < states ? rows - 1 : states;
}

// ---- the stream kernel on the wide walk (stream.hip, round 6) ------------------------------------------------------------
// The stream kernel keeps the positions of a sub-task's strings in LDS, per wave -- with the wide walk's image beside them:
// sub-tasks of 640 strings (42 KB for 16 waves) and an image of its own with a SMALLER TIER, the first `StreamWideTier` states
// of the same numbering (entries that lead beyond it are the escape state's; a zipped image keeps its rows and drops headers).
constexpr uint32_t kStreamWideStrings = 640;   // at least (a zipped image that leaves more room gets larger sub-tasks, stream.hip)
constexpr uint32_t kStreamWideStageBytes = 16 * (kStreamWideStrings + 16) * 4;   // kStreamWaves waves
inline uint32_t StreamWideTier(uint32_t letters, uint32_t regexps, uint32_t wide, uint32_t zipFull)
{
	if (!wide)
		return 0;
	const uint32_t r = regexps <= kMaxLdsCountRegexps ? regexps : 0;
	const uint32_t budget = kLdsPerBlock - kStreamWideStageBytes - 64;
	if (MakeWideLayout(zipFull ? zipFull : 1, letters, r, zipFull).total > budget)
		return 0;   // (a zipped image whose rows alone do not leave the room)
	uint32_t lo = zipFull ? zipFull : 1, hi = wide;   // the largest tier whose layout fits (the layout grows with the tier)
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1) / 2;
		if (MakeWideLayout(mid, letters, r, zipFull).total <= budget)
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

// Host-side, fully decoded scanner.  States are in the REFERENCE's numbering ("orig") unless a name says perm.
struct HostTable {
	// geometry (mirrors Scanner::Locals, multi.h:315-323)
	uint32_t states = 0, letters = 0, regexps = 0, initial = 0;
	bool empty = false;
	bool ranked = true;               // false: hot / permutation / dense rows not computed yet (EnsureRanked)
	uint32_t scannerType = 1;         // ScannerIOTypes (common.h:34-40): 1 Scanner, 2 SimpleScanner
	uint32_t headerSize = 0, rowStride = 0;
	uint64_t refBufSize = 0;
	uint64_t blobBytes = 0;           // bytes of the serialised image this scanner occupied (what Mmap() would consume)

	std::vector<uint16_t> cls;        // [264] letter class of each Char (Translate() - HEADER_SIZE)
	std::vector<uint32_t> next;       // [states * letters] next state index, orig numbering
	std::vector<uint8_t> flags;       // [states] kFinal|kDead|kAbsorbing
	std::vector<uint64_t> acceptOff;  // [states + 1] CSR into acceptIds
	std::vector<uint64_t> acceptIds;  // AcceptedRegexps lists (multi.h:149-158)

	// device numbering: hot states first ("perm" ids).  permOfOrig / origOfPerm are inverse permutations.
	std::vector<uint32_t> permOfOrig, origOfPerm;
	uint32_t hot = 0;                 // number of states with a dense LDS row; trap id == hot
	uint32_t hotFinalLo = 0;          // hot perm ids >= this are Final (the hot set is ordered non-final first)
	uint32_t hotDeadLo = 0;           // hot perm ids in [hotDeadLo, hotFinalLo) are Dead (ordered plain, Dead, Final)
	float deadShare = 0, finalShare = 0;   // share of the byte model's visits that fall on Dead / Final states
	float topShare = 1;               // share of the ranking's mass on its most visited state (1 = all lanes in one row)
	// steps (text bytes only, capped at 255) from every state to the nearest Final / Final-or-Dead state: the ragged
	// kernel with actions skips the exact re-walk of a trapped chunk that cannot reach one (table.cpp EnsureActDist)
	std::vector<uint8_t> distFinal, distFlagged;   // [states], reference numbering; empty until first needed
	bool incPacked = false;           // regexps <= 8 and every final-list multiplicity <= 255: inc64 is usable
	std::vector<uint64_t> inc64;      // [states] (orig numbering) byte r = how often regexp r is in the final list
	uint32_t compact = 0;             // perm ids [0, compact) also have a class-indexed u16 row in LDS (tiled/ragged kernels)
	uint32_t wide = 0;                // perm ids [0, wide) have a row in the wide walk's LDS image (wide.hip; 0 = no such image)
	uint32_t zipFull = 0;             // != 0: the wide image is ZIPPED (MakeWideLayout): perm ids [0, zipFull) have a row of their own,
	                                  // [zipFull, wide) a header + <= 3 exceptions against the row of zipBase[id - zipFull]
	std::vector<uint16_t> zipBase;    // [wide - zipFull] perm id (< zipFull) of that row
	float offsetBatchShare = 0;       // share of the bytes scanned since the last ranking that came as offset batches (one string per
	                                  // lane: the zipped step's 20 vector instructions bound that kernel, table.cpp ChooseZip)
	float zipPlainOutside = 0;        // what the plan that chose between the two images estimated: share of the ranking's mass outside
	float zipOutside = 0;             // the plain rows / outside the zipped tier (table.cpp ChooseZip)
	float outsideDense = 0;           // share of the ranking's mass on states WITHOUT a dense row / ...
	float outsideWide = 0;            // ... without a wide row (from the byte model until adapt() has seen scans, then measured)
	bool massMeasured = false;        // those shares come from visit counters, not from the a-priori byte model
	float wideTwiceShare = 0;         // share of the wide walk's 16-byte wave-chunks it walked twice (exact, between the two most
	                                  // recent adapt() calls)
	std::vector<uint8_t> hotRows;     // [(hot + 1) * 256] u8: next perm id (< hot) or `hot` (= leaves the hot set)
	std::vector<uint8_t> hotFlags;    // [256] flags of hot perm ids (kAbsorbing used for the early-out ballot)
	std::vector<double> seenMass;     // [states] what the scans so far visited (lane-steps, halved at every adapt(); orig numbering)
	std::vector<double> priorMass;    // [states] expected visits under the byte model, max-normalised (orig numbering)
	uint64_t lastTrapSamples = 0;     // cold-state samples seen by the most recent pire_hip_table_adapt()
	uint64_t lastWideTrapChunks = 0;  // 16-byte wave-chunks the wide walk walked twice, as seen by the most recent adapt() (exact)
	uint32_t adaptations = 0;
};

// Everything the end of a string needs, in ONE 16-byte load: reference StateIndex, device id + flags, regexp mask.
struct FinRec {
	uint32_t orig;        // StateIndex (multi.h:281-284) of the end state
	uint32_t permFlags;   // device id of the end state | flags << 28
	uint64_t acceptMask;  // bit r = regexp r in AcceptedRegexps() (regexps <= 64)
};

// Device image (one HIP device).
struct DeviceTable {
	int device = -1;
	uint8_t* hotRows = nullptr;       // [(hot+1)*256]
	uint8_t* hotRowsRot = nullptr;    // the same rows with their columns in rotated byte order (RotColumn)
	uint8_t* hotFlags = nullptr;      // [256]
	uint16_t* cls = nullptr;          // [264]
	uint32_t* nextPerm = nullptr;     // [states*letters], perm ids in, perm ids out
	uint8_t* flagsPerm = nullptr;     // [states]
	uint32_t* origOfPerm = nullptr;   // [states]
	uint32_t* permOfOrig = nullptr;   // [states]
	uint64_t* acceptMaskPerm = nullptr;  // [states] bit r = regexp r accepted (regexps <= 64), else null
	uint64_t* acceptOffPerm = nullptr;   // [states+1] CSR (regexps > 64)
	uint64_t* acceptIds = nullptr;
	struct FinRec* finSelf = nullptr; // [states] end-of-string record when End() is not requested
	struct FinRec* finEnd = nullptr;  // [states] end-of-string record after Step(EndMark)
	uint64_t* incPerm = nullptr;      // [states] packed per-regexp increments of HalfFinalScanner::TakeAction, or null
	uint8_t* distFinalPerm = nullptr;    // [states] HostTable::distFinal by device id (uploaded when first needed)
	uint8_t* distFlaggedPerm = nullptr;
	uint16_t* compactRows = nullptr;  // [(compact+1) rows] LDS address / 4 of the next state's row (last row = escape), padded
	uint16_t* wideRows = nullptr;     // [(wide+1) rows] the wide walk's LDS image (WideLayout), or null
	uint16_t* next16 = nullptr;       // [states*letters] nextPerm as u16 when states <= 65536 (half the L2 footprint), or null
	uint16_t* wideRowsStream = nullptr;   // the wide image once more with the stream kernel's smaller tier (StreamWideTier), or null
	uint32_t wideStream = 0;          // ... its tier
	uint32_t* visitWide = nullptr;    // [wide+1] sampled visits of the wide rows (one lane per wave per 128-byte tile)
	uint32_t* visitHot = nullptr;     // [256]    sampled visits of hot perm ids (one lane per wave per tile)
	uint32_t* visitCold = nullptr;    // [states] trapped chunks that ended in this (cold) perm id
	unsigned long long* workCounter = nullptr;   // [kWorkSlots] ragged kernel: next string range to hand out;
	                                             // one slot per launch so that launches on different streams
	                                             // never share a counter
	// Auto-adaptation signal: blocks that saw traps add them to visitHot[kTrapSlot] (device atomics) and store the new
	// total into this word of MAPPED HOST memory (a plain system-scope store: PCIe atomics are not needed, and a
	// late smaller value only delays the trigger), so the host can look at it at every launch without synchronising.
	volatile uint32_t* trapSignalHost = nullptr;
	uint32_t* trapSignalDev = nullptr;
	uint64_t bytes = 0;
};

}  // namespace pirehip

namespace pirehip {
constexpr uint32_t kWorkSlots = 1024;
// The ragged kernels take ranges of strings from a counter that must be zero when a launch starts.  Launch number k of a
// table on a device uses slot k % kWorkSlots = two words {next string, blocks done}: every block adds 1 to `done` when
// it leaves, and the block that finds itself last puts BOTH words back to zero -- so a slot is clean whenever no launch
// is using it, whatever kinds of launches (tiled, generic, failed, n == 0) took slot numbers in between, and no launch
// pays a memset dispatch of its own (5 us in front of every ragged kernel).  Round 2 had launch k clear the slot of
// launch k + kWorkSlots instead, which left a slot dirty when that later launch number went to a kernel that does not
// clear.  The array is zeroed when the image is uploaded.
inline unsigned long long* WorkSlotOf(unsigned long long* base, uint32_t k)
{
	return base + 2 * (k % kWorkSlots);
}
}  // namespace pirehip

namespace pirehip { constexpr int kMaxDevices = 64; }

namespace pirehip {
// HalfFinalScanner counting on CountingRowKernel (counting.hip): the table as letter-indexed rows with the increments
// of the TARGET state as the step's action, reference numbering (adaptation does not touch it); built when first needed.
struct HalfRowsHost {
	bool tried = false;
	uint32_t nreg = 0, initialAct = 0, maxLen = 65000;
	std::vector<uint32_t> lrows, lactWords;   // as CountingHost::lrows / lactWords
	std::vector<uint8_t> letterOf, finalTag;  // [264] letter of every Char; [states] bit 0 = Final
};
struct HalfRowsDevice {
	int device = -1;
	uint32_t* lrows = nullptr;
	uint32_t* lactWords = nullptr;
	uint8_t* letterOf = nullptr;
	uint8_t* finalTag = nullptr;
};
// pire_hip_select (select.hip): per state, by REFERENCE state index, the W = max(1, ceil(regexps / 64)) words of its
// AcceptedRegexps() mask and its Final flag.  A re-ranking (pire_hip_table_adapt, the automatic ones, a swap in the
// background) renumbers the DEVICE ids and nothing else, so this image is built once per table, uploaded once per device
// and never touched again: the adaptation paths do not know it exists.  (FinRec::acceptMask behind permOfOrig holds the
// same bits for <= 64 regexps -- in the numbering that does change under a swap.)
struct SelectHost {
	bool built = false;
	uint32_t words = 1;
	std::vector<uint64_t> masks;   // [states * words]
	std::vector<uint8_t> fin;      // [states]
};
struct SelectDevice {
	int device = -1;
	uint64_t* masks = nullptr;
	uint8_t* fin = nullptr;
};
}  // namespace pirehip

struct pire_hip_table {
	pirehip::HostTable host;
	pirehip::HalfRowsHost halfRows;
	pirehip::HalfRowsDevice halfRowsDev[pirehip::kMaxDevices];
	std::mutex halfRowsMutex;
	pirehip::SelectHost select;
	pirehip::SelectDevice selectDev[pirehip::kMaxDevices];
	std::mutex selectMutex;
	// One image per HIP device (devs[d].device == d once uploaded), so that one handle serves every GPU of the node,
	// from one host thread or from several.  Guarded by uploadMutex; the run entry points COPY the image's pointers
	// while holding it (UploadTable) and never look at devs[] afterwards.
	pirehip::DeviceTable devs[pirehip::kMaxDevices];
	std::mutex uploadMutex;
	std::vector<pirehip::DeviceTable> retired;   // images an AUTOMATIC adaptation replaced: alive until destroy (captured graphs)
	std::atomic<uint32_t> workSlot[pirehip::kMaxDevices] = {};   // per device image: round-robin over its counter pairs
	std::mutex segMutex;
	std::vector<uint32_t> segModes;      // segmented.hip: mode representatives (state indices) earlier calls learned
	// segmented.hip, ModeFunction: for a pair (start state, mode representative), reference numbering, the function f
	// with "mode's state = f(mode 0's state)" after any text -- or an empty vector when there is none
	struct SegModeFn {
		uint32_t a0, b0, minSteps;
		std::vector<uint32_t> f;
	};
	std::vector<SegModeFn> segModeFns;
	// segmented.hip, EnsureModeProduct: the product automaton of this table started in (a0, b0) -- the walk of two
	// modes as ONE walk -- with the two components of every product state (reference numbering, both)
	std::unique_ptr<pire_hip_table> segProduct;
	uint32_t segProductA0 = 0, segProductB0 = 0;
	bool segProductTried = false;
	std::vector<uint32_t> segProductA, segProductB;
	// Adaptation (table.cpp AdaptTable) rewrites host.{hot, origOfPerm, permOfOrig, hotRows, ...} and replaces the images.
	// Run entry points hold adaptMutex SHARED from their first look at the table until they return (internal.h TableUse);
	// an adaptation -- the caller's or the automatic one -- holds it exclusively, drains the devices and frees the old
	// images: no call can be between "copied the pointers" and "enqueued its kernels" at that moment.
	std::shared_mutex adaptMutex;
	std::atomic<uint32_t> autoAdapts{0};
	std::atomic<uint64_t> wideLaunched{0};   // wave-chunks handed to the wide walk since the last adapt()
	std::atomic<uint64_t> bytesScanned{0};   // text bytes handed to the kernels of pire_hip_run[_strided] since the last ranking (where the host knows)
	std::atomic<uint64_t> bytesNominal{0};   // ... the same with 48 bytes a string where it does not (offsets on the device), and
	std::atomic<uint64_t> bytesOffsetBatches{0};   // those of them that came as offset batches (the ragged / stream kernels): what
	                                               // ChooseZip weighs the zipped image by (HostTable::offsetBatchShare)
	// the adaptation a call that only enqueues starts in the background (table.cpp BackgroundAdaptStep): state 0 idle, 1 the
	// worker is on its way, 2 `host` + `image` (device `device`) are ready to be swapped in at a launch boundary
	struct Background {
		std::mutex mutex;                 // start / join / swap, one at a time
		std::thread thread;
		std::atomic<int> state{0};
		std::unique_ptr<pirehip::HostTable> host;
		pirehip::DeviceTable image;
		int device = -1;
		uint64_t trapsAtLastLook = 0;     // the trap signal when a worker last found nothing to do
		std::atomic<uint32_t> swaps{0};
	} bg;
	// pire_hip_table_config_set(): this table's own configuration (a second user of the library in the same process -- another
	// component, another thread pool -- sets the process-wide one for itself).  Written under adaptMutex held
	// exclusively, read by the entry points under TableUse.
	bool hasConfig = false;
	pire_hip_config config = {};
	std::atomic<uint32_t> selfTested[pirehip::kMaxDevices] = {};   // per device, bit k: Dispatch's kernel kind k passed its known-answer
	                                                               // batch on this table there (api.cpp SelfTest); bits 8-11: the
	                                                               // entry points with actions (api.cpp SelfTestPrefix, ...)
};
namespace pirehip {
// The bits of pire_hip_table::selfTested whose kernels take a different instantiation on a zipped wide image (wide, ragged_wide,
// stream_wide and the entry points with actions, whose variants include the wide walk): a ranking that zips the image or gives the
// plain rows back clears them on every device (ForgetLayoutSelfTests), and the next call of each kind is tested again.  A ranking
// that keeps the layout keeps them: a background swap may land inside a timed loop.
constexpr uint32_t kSelfTestedOnWideImage = (1u << 2) | (1u << 4) | (1u << 6) | (0xFu << 8);
inline void ForgetLayoutSelfTests(pire_hip_table* t)
{
	for (auto& bits : t->selfTested)
		bits.fetch_and(~kSelfTestedOnWideImage);
}
}  // namespace pirehip
namespace pirehip { constexpr uint32_t kMaxAutoAdapts = 6; }

namespace pirehip {

// Kernel parameter block (passed by value).
struct ScanParams {
	// table
	const uint8_t* hotRows;
	const uint8_t* hotRowsRot;   // host side only (LaunchTiled swaps it in for the rotated-column kernel)
	float topShare;              // host side only: share of the walk's steps the most visited state carries (ranking's estimate)
	const uint8_t* hotFlags;
	const uint16_t* cls;
	const uint32_t* nextPerm;
	const uint8_t* flagsPerm;
	const uint32_t* origOfPerm;
	const uint32_t* permOfOrig;
	const uint64_t* acceptMaskPerm;
	const uint64_t* acceptOffPerm;
	const uint64_t* acceptIds;
	const FinRec* finSelf;
	const FinRec* finEnd;
	uint32_t* visitHot;
	uint32_t* visitCold;
	uint32_t* trapSignal;   // mapped host word (device address) for the auto-adaptation policy, or null
	const uint16_t* compactRows;
	uint32_t compact;        // 0 = tier off
	const uint16_t* wideRows;   // nullable: the wide walk's LDS image
	const uint16_t* next16;     // nullable
	uint32_t* visitWide;
	uint32_t wide;              // states with a wide row; 0 = no image
	uint32_t zipFull;           // != 0: the image is zipped (internal.h MakeWideLayout), this many states have a row of their own
	uint32_t wideOutSlot;       // visitWide[wideOutSlot] counts the visit samples that found their lane outside the tier (== wide,
	                            // except under the stream kernel's image, whose tier is a prefix of the table's)
	const uint16_t* wideRowsStream;   // host side only: the stream kernel's image (LaunchStreamWide swaps it in) and its tier
	uint32_t wideStream;
	float outsideDense, outsideWide;   // host side only: LaunchTiled's choice between the dense and the wide walk
	uint32_t forceLanes;               // host side only: 1 / 2 = LaunchWide takes the kernel with that many strings per lane (the self-test)
	std::atomic<uint64_t>* wideLaunched;   // host side only: wave-chunks handed to the wide walk since the last adapt()
	bool massMeasured;                 // host side only
	const uint64_t* incPerm; // nullable
	uint32_t hotFinalLo;
	uint32_t hotDeadLo;
	float deadShare, finalShare;   // host-side hints for the choice of kernel (any choice is correct)
	const uint8_t* actDist;        // nullable: steps to the nearest state the action cares about (ragged kernel with actions)
	uint32_t states, letters, regexps, hot;
	uint32_t startPerm;      // perm id every string starts in (Initialize(), then Begin() if requested)
	uint32_t beginCls, endCls;
	uint32_t flags;          // PIRE_HIP_RUN_*
	// batch
	const uint8_t* text;
	const uint64_t* offsets; // nullable: then string i = [i*stride, i*stride+len)
	const uint64_t* ends;    // nullable: string i = [offsets[i], ends[i]) -- strings may overlap or leave gaps (the
	                         // segments of segmented.hip); then textEnd = bytes readable at `text`
	uint64_t textEnd;
	uint64_t n, len, stride;
	const uint32_t* initIdx; // nullable
	uint32_t* outIdx;        // nullable
	uint8_t* outFinal;       // nullable
	unsigned long long* outCounts;  // nullable
	unsigned long long* workBase;   // host side only: the ring of ragged work counters of the image in use
	int workDevice;                 // host side only: the device of that image (its launch counter, internal.h WorkSlotOf)
	// HalfFinalScanner on the ragged kernel: the state every string starts its text in (device id) and the counts
	// Initialize() [+ Step(BeginMark)] have already taken (half_final.h:137-164) -- the same for every string, so the
	// host walks those two steps once instead of every lane doing them (two dependent loads) for every string
	uint32_t hfStart;
	uint32_t hfStartC[8];
	// host side only, filled by FillParams under the entry point's TableUse (below) and valid while it is held: the
	// numbering of the image the pointers above belong to, and that image's distance tables when the entry point asked
	// for them.  What an entry point derives after FillParams (start states of the half-final / suffix / segmented
	// scans, mode representatives) goes through these.
	const uint32_t* hostPermOfOrig;
	const uint32_t* hostOrigOfPerm;
	pire_hip_table* owner;          // the table itself (the first-use self-test walks its host image)
	const uint8_t* distFinalPerm;
	const uint8_t* distFlaggedPerm;
#ifdef PIRE_HIP_TUNING
	unsigned long long* stamps;     // timing experiments: [blocks][4] wall-clock stamps (start, table loaded, walk done, end)
#endif
};

__host__ __device__ inline uint32_t CompactBytes(const ScanParams& p)
{
	return p.compact ? (p.compact + 1) * CompactPitch(p.letters) : 0;
}

// The library configuration (include/pire_hip.h pire_hip_config): a snapshot by value, taken once per call.
pire_hip_config GetConfig();
void SetError(const std::string& msg);
// Inside a catch (...) of an extern "C" entry point: std::bad_alloc / std::length_error (blob fields that ask for
// absurd sizes) -> PIRE_HIP_ENOMEM, anything else -> PIRE_HIP_EINVAL; the message goes to pire_hip_last_error().
int HandleException() noexcept;
int HipFail(hipError_t e, const char* what);   // sets the error, returns PIRE_HIP_ENODEVICE / ENOMEM

// One block of stream-ordered scratch (hipMallocAsync), freed on the same stream when the owner leaves its scope: declare
// it in the scope that encloses every launch using the block, and the free is ordered behind those launches on every
// path out.  Where a block outlives the function that allocates it, the caller passes the owner in.
class StreamScratch {
	void* p = nullptr;
	hipStream_t stream;

public:
	explicit StreamScratch(hipStream_t s) : stream(s) {}
	StreamScratch(const StreamScratch&) = delete;
	StreamScratch& operator=(const StreamScratch&) = delete;
	~StreamScratch()
	{
		if (p)
			(void)hipFreeAsync(p, stream);
	}
	int Alloc(size_t bytes, const char* what)   // once per owner
	{
		const hipError_t e = hipMallocAsync(&p, bytes, stream);
		if (e == hipSuccess)
			return PIRE_HIP_OK;
		p = nullptr;
		return HipFail(e, what);
	}
	void* get() const { return p; }
	template <class T>
	T* as() const { return static_cast<T*>(p); }
};

// What every entry point asks of a batch whose arrays the HOST can read: offsets that do not decrease, and text behind
// them unless every string is empty (a null text pointer is fine then, tests/pire_ut.cpp:832-837).
inline int CheckOffsets(const uint64_t* offsets, uint64_t n)
{
	for (uint64_t i = 0; i < n; ++i)
		if (offsets[i] > offsets[i + 1]) {
			SetError("offsets must be non-decreasing");
			return PIRE_HIP_EINVAL;
		}
	return PIRE_HIP_OK;
}
// offsets == nullptr: n records of `len` bytes, `stride` apart.  *textBytes: what is read at `text`.
inline int CheckHostBatch(const void* text, const uint64_t* offsets, uint64_t n, uint64_t len, uint64_t stride, uint64_t* textBytes)
{
	if (offsets)
		if (int rc = CheckOffsets(offsets, n))
			return rc;
	*textBytes = offsets ? offsets[n] : n ? (n - 1) * stride + len : 0;
	if (!text && *textBytes) {
		SetError("null text pointer with non-empty strings");
		return PIRE_HIP_EINVAL;
	}
	return PIRE_HIP_OK;
}

// Owns the temporary device buffers of a host-pointer call (PCIe-inclusive convenience mode).  Default: blocks from the
// per-device cache of api.cpp (StagingAcquire / StagingRelease: no allocation in steady state); they go back when the
// call returns -- after its stream has been drained, which the destructor sees to itself: an error path may leave
// copies or kernels in flight.  pire_hip_config.host_staging: 1 = hipMalloc + hipFree per call (round 2), 2 = the
// stream-ordered pool.  The entry points reach it through BatchIO (below), which is also where a call's pointers pass
// through untouched when they are the device's already.
int StagingAcquire(size_t bytes, void** out, size_t* blockBytes);
void StagingRelease(void* p, size_t blockBytes);
// the same for PINNED host blocks: small inputs and results cross PCIe from / into pinned memory (a copy between
// pageable memory and the device goes through the runtime's own staging and costs 10-15 us a piece, which is most of
// a 10-string call), and the caller's pageable arrays are touched with plain memcpy
int StagingAcquireHost(size_t bytes, void** out, size_t* blockBytes);
void StagingReleaseHost(void* p, size_t blockBytes);
struct Staging {
	std::vector<void*> ptrs, hostPtrs;
	std::vector<size_t> sizes, hostSizes;
	struct Deferred {
		void* dst;
		const void* pinned;
		size_t bytes;
	};
	std::vector<Deferred> deferred;   // results waiting in pinned blocks for Finish()
	// Small calls (round 3): every input and result of the call is carved out of ONE device block and its pinned twin
	// (same offsets), so that the inputs cross PCIe in one copy and the results in one -- two copies enqueued per call
	// instead of four to six, at 4-5 us of stream time each (profiles/r03_small_call_timeline.log).  Inputs wait in the
	// pinned block until Flush() (called by the first Alloc() / Out() / Finish() at the latest: every user stages its
	// inputs first, then its result arrays, then launches); results are fetched by Finish().
	static constexpr size_t kArenaBytes = size_t(256) << 10;
	uint8_t* arenaDev = nullptr;
	uint8_t* arenaPin = nullptr;
	size_t arenaUsed = 0, arenaInputs = 0, arenaFlushed = 0;
	bool arenaTried = false;
	struct ArenaOut {
		void* dst;
		size_t off, bytes;
	};
	std::vector<ArenaOut> arenaOuts;
	hipStream_t stream = nullptr;
	uint32_t mode = 1;   // a default-constructed Staging is round 2's
	bool drained = false;
	static constexpr size_t kPinnedMax = size_t(1) << 20;   // larger pieces go straight from / to the caller's memory
	Staging() {}
	explicit Staging(hipStream_t s) : stream(s), mode(GetConfig().host_staging) {}
	~Staging()
	{
		if (mode == 0 && !drained && (!ptrs.empty() || !hostPtrs.empty()))
			(void)hipStreamSynchronize(stream);
		for (size_t i = 0; i < ptrs.size(); ++i) {
			if (mode == 0)
				StagingRelease(ptrs[i], sizes[i]);
			else if (mode == 2)
				(void)hipFreeAsync(ptrs[i], stream);
			else
				(void)hipFree(ptrs[i]);
		}
		for (size_t i = 0; i < hostPtrs.size(); ++i)
			StagingReleaseHost(hostPtrs[i], hostSizes[i]);
	}
	// a piece of the arena, or null when the call is not a small one (any more)
	uint8_t* Carve(size_t bytes)
	{
		if (mode != 0)
			return nullptr;
		if (!arenaTried) {
			arenaTried = true;
			void *d = nullptr, *h = nullptr;
			if (Alloc(&d, kArenaBytes, /*fromArena=*/false) != PIRE_HIP_OK || Pinned(&h, kArenaBytes) != PIRE_HIP_OK)
				return nullptr;
			arenaDev = static_cast<uint8_t*>(d);
			arenaPin = static_cast<uint8_t*>(h);
		}
		const size_t need = (std::max<size_t>(bytes, 16) + 255) & ~size_t(255);
		if (!arenaDev || !arenaPin || arenaUsed + need > kArenaBytes)
			return nullptr;
		uint8_t* p = arenaDev + arenaUsed;
		arenaUsed += need;
		return p;
	}
	// the inputs staged so far: one copy
	int Flush()
	{
		if (arenaInputs > arenaFlushed) {
			const hipError_t e = hipMemcpyAsync(arenaDev + arenaFlushed, arenaPin + arenaFlushed, arenaInputs - arenaFlushed,
			                                    hipMemcpyHostToDevice, stream);
			if (e != hipSuccess)
				return HipFail(e, "hipMemcpy(H2D)");
			arenaFlushed = arenaInputs;
		}
		return PIRE_HIP_OK;
	}
	int Alloc(void** out, size_t bytes, bool fromArena = true)
	{
		*out = nullptr;
		if (fromArena) {
			if (int rc = Flush())
				return rc;
			if (uint8_t* p = Carve(bytes)) {
				*out = p;
				return PIRE_HIP_OK;
			}
		}
		size_t block = bytes ? bytes : 16;
		if (mode == 0) {
			if (int rc = StagingAcquire(block, out, &block))
				return rc;
		} else {
			const hipError_t e = mode == 2 ? hipMallocAsync(out, block, stream) : hipMalloc(out, block);
			if (e != hipSuccess)
				return HipFail(e, "hipMalloc(staging)");
		}
		ptrs.push_back(*out);
		sizes.push_back(block);
		return PIRE_HIP_OK;
	}
	int Pinned(void** out, size_t bytes)
	{
		size_t block = 0;
		if (int rc = StagingAcquireHost(bytes, out, &block))
			return rc;
		hostPtrs.push_back(*out);
		hostSizes.push_back(block);
		return PIRE_HIP_OK;
	}
	template <class T>
	int In(const T* host, size_t count, const T** dev, hipStream_t s)
	{
		void* d;
		const size_t bytes = count * sizeof(T);
		if (s == stream && arenaInputs == arenaUsed)   // inputs only in front of everything else of the arena
			if (uint8_t* p = Carve(bytes)) {
				if (bytes)   // (an empty input may come with a null pointer: memcpy's arguments are declared non-null, UBSan r4)
					memcpy(arenaPin + (p - arenaDev), host, bytes);
				arenaInputs = arenaUsed;
				*dev = reinterpret_cast<const T*>(p);
				return PIRE_HIP_OK;
			}
		if (int rc = Alloc(&d, bytes, /*fromArena=*/false))
			return rc;
		if (count) {
			const void* src = host;
			if (mode == 0 && bytes <= kPinnedMax) {
				void* pin = nullptr;
				if (int rc = Pinned(&pin, bytes))
					return rc;
				memcpy(pin, host, bytes);
				src = pin;
			}
			hipError_t e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, s);
			if (e != hipSuccess)
				return HipFail(e, "hipMemcpy(H2D)");
		}
		*dev = static_cast<const T*>(d);
		return PIRE_HIP_OK;
	}
	// Result `bytes` from device memory into the caller's array: enqueued now, in the caller's array after Finish()
	int Out(void* hostDst, const void* dev, size_t bytes)
	{
		if (!bytes || !hostDst)
			return PIRE_HIP_OK;
		if (int rc = Flush())
			return rc;
		const uint8_t* dp = static_cast<const uint8_t*>(dev);
		if (arenaDev && dp >= arenaDev && dp + bytes <= arenaDev + kArenaBytes) {
			arenaOuts.push_back(ArenaOut{hostDst, size_t(dp - arenaDev), bytes});
			return PIRE_HIP_OK;
		}
		void* dst = hostDst;
		if (mode == 0 && bytes <= kPinnedMax) {
			void* pin = nullptr;
			if (int rc = Pinned(&pin, bytes))
				return rc;
			deferred.push_back(Deferred{hostDst, pin, bytes});
			dst = pin;
		}
		const hipError_t e = hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, stream);
		return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemcpy(D2H)");
	}
	// Drain the stream, then hand the results that waited in pinned blocks to the caller's arrays
	int Finish()
	{
		if (int rc = Flush())
			return rc;
		if (!arenaOuts.empty()) {
			size_t lo = kArenaBytes, hi = 0;
			for (const ArenaOut& o : arenaOuts) {
				lo = std::min(lo, o.off);
				hi = std::max(hi, o.off + o.bytes);
			}
			const hipError_t ce = hipMemcpyAsync(arenaPin + lo, arenaDev + lo, hi - lo, hipMemcpyDeviceToHost, stream);
			if (ce != hipSuccess)
				return HipFail(ce, "hipMemcpy(D2H)");
		}
		const hipError_t e = hipStreamSynchronize(stream);
		if (e != hipSuccess)
			return HipFail(e, "copy back / synchronize");
		drained = true;
		for (const Deferred& d : deferred)
			memcpy(d.dst, d.pinned, d.bytes);
		deferred.clear();
		for (const ArenaOut& o : arenaOuts)
			memcpy(o.dst, arenaPin + o.off, o.bytes);
		arenaOuts.clear();
		return PIRE_HIP_OK;
	}
};

// The pointers of ONE call of a batch entry point, whichever side they live on: with PIRE_HIP_RUN_ON_DEVICE they pass
// through, otherwise they are checked (CheckHostBatch) and staged (Staging).  The entry point fills its parameters from
// what this hands back, launches once and returns Finish().  Order of a call: Text(), further In()s, Result()s, Ready(),
// the launches, Finish() -- which is Staging's order (inputs, result arrays, Flush, launches, Outs, Finish), so a small
// call crosses PCIe in one copy each way.
struct BatchIO {
	const hipStream_t stream;
	std::optional<Staging> st;   // of a host-pointer call; a device-pointer call has none
	struct Back {
		void* host;
		const void* dev;
		size_t bytes;
	};
	std::vector<Back> backs;   // results to copy back, in the order they were asked for
	BatchIO(hipStream_t s, bool onDevice) : stream(s)
	{
		if (!onDevice)
			st.emplace(s);
	}
	// offsets == nullptr: fixed-length records (len, stride)
	int Text(const void* text, const uint64_t* offsets, uint64_t n, uint64_t len, uint64_t stride, const uint8_t** dText,
	         const uint64_t** dOffsets)
	{
		*dText = static_cast<const uint8_t*>(text);
		*dOffsets = offsets;
		if (!st)
			return PIRE_HIP_OK;
		uint64_t textBytes = 0;
		if (int rc = CheckHostBatch(text, offsets, n, len, stride, &textBytes))
			return rc;
		if (int rc = st->In(static_cast<const uint8_t*>(text), size_t(textBytes), dText, stream))
			return rc;
		return offsets ? st->In(offsets, size_t(n) + 1, dOffsets, stream) : PIRE_HIP_OK;
	}
	template <class T>
	int In(const T* host, size_t count, const T** dev)
	{
		*dev = host;
		return st ? st->In(host, count, dev, stream) : PIRE_HIP_OK;
	}
	// `bytes` at `dev` into the caller's `host` array when the call finishes (host-pointer calls; nothing when host is null)
	void CopyBack(void* host, const void* dev, size_t bytes)
	{
		if (st)
			backs.push_back(Back{host, dev, bytes});
	}
	// A result array of allocCount elements on the device -- the caller's own when that is where it lives -- of which
	// the first copyCount come back (the two differ where a kernel wants room that nobody reads: a table of no regexps)
	template <class T>
	int Result(T* caller, size_t allocCount, size_t copyCount, T** dev)
	{
		*dev = caller;
		if (!st)
			return PIRE_HIP_OK;
		void* d = nullptr;
		if (int rc = st->Alloc(&d, allocCount * sizeof(T)))
			return rc;
		*dev = static_cast<T*>(d);
		CopyBack(caller, d, copyCount * sizeof(T));
		return PIRE_HIP_OK;
	}
	// In front of the first launch: the inputs that still wait in the staging arena go to the device now.  (A Result()
	// sends them too, but a call may have none: pire_hip_slow_run with out_counts alone.)
	int Ready() { return st ? st->Flush() : PIRE_HIP_OK; }
	int Finish()
	{
		if (!st)
			return PIRE_HIP_OK;
		for (const Back& b : backs)
			if (int rc = st->Out(b.host, b.dev, b.bytes))
				return rc;
		return st->Finish();
	}
};

// PIRE_HIP_RUN_HOST_OFFSETS: the text is resident, the offsets are the host's.  They are checked, copied into
// stream-ordered scratch and handed to `body` (which launches); the stream is drained on success, because the caller's
// array was the source of an asynchronous copy.
template <class Body>
int WithOffsetsOnDevice(const uint64_t* offsets, uint64_t n, hipStream_t stream, Body&& body)
{
	if (int rc = CheckOffsets(offsets, n))
		return rc;
	{
		StreamScratch d(stream);
		if (int rc = d.Alloc((n + 1) * 8, "hipMallocAsync(offsets)"))
			return rc;
		const hipError_t e = hipMemcpyAsync(d.get(), offsets, (n + 1) * 8, hipMemcpyHostToDevice, stream);
		if (e != hipSuccess)
			return HipFail(e, "hipMemcpy(offsets)");
		if (int rc = body(d.as<const uint64_t>()))
			return rc;
	}
	const hipError_t e = hipStreamSynchronize(stream);
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipStreamSynchronize");
}

// table.cpp
int BuildHostTable(const void* blob, size_t len, HostTable* out);
int UploadTable(pire_hip_table* t, DeviceTable* image);   // image of the CURRENT device (built on first use), copied out
int BuildDeviceImage(const HostTable& h, int dev, DeviceTable* out);   // allocations + copies of a ranked table's image, current device
void JoinBackgroundAdapt(pire_hip_table* t);   // waits for an adaptation in the background and drops what it prepared
void EnsureRanked(pire_hip_table* t);
std::vector<uint16_t> BuildWideRows(const HostTable& h, uint32_t tier = 0);   // the wide walk's LDS image (WideLayout), current numbering; tier != 0: of the first `tier` states only
// after UploadTable, current device: the per-state distance tables (built on first use)
int EnsureActDist(pire_hip_table* t, const uint8_t** distFinalPerm, const uint8_t** distFlaggedPerm);
void FreeAllDeviceTables(pire_hip_table* t);
struct GlueProduct {
	std::vector<std::pair<uint32_t, uint32_t>> states;   // numbered product states (lhs state, rhs state)
	std::vector<uint32_t> next;                          // [states * letters]
	bool failed = false;                                 // more than maxSize new states: the glue yields an empty scanner
};
int GlueBfsHost(const HostTable& a, const HostTable& b, const std::vector<uint32_t>& la, const std::vector<uint32_t>& lb,
                size_t maxSize, GlueProduct* out);
int GlueBfsDevice(const HostTable& a, const HostTable& b, const std::vector<uint32_t>& la,
                  const std::vector<uint32_t>& lb, size_t maxSize, GlueProduct* out);   // glue.hip
int GlueHostTables(const HostTable& a, const HostTable& b, size_t maxSize, HostTable* out, bool onDevice = false);
int AdaptTable(pire_hip_table* t, uint32_t* changedRows, bool automatic = false);
// the auto-adaptation policy (pire_hip_config.auto_adapt): called at every launch boundary, cheap when nothing is due
void MaybeAutoAdapt(pire_hip_table* t, bool enqueueOnly = false);
int CheckFailures(pire_hip_table* t, uint64_t* out);
void FreeDeviceTable(DeviceTable* d);

// tiled.hip / ragged.hip / exact.hip / corpus.hip
int LaunchGeneric(const ScanParams& p, hipStream_t stream);
// what a kernel of whole tasks leaves over: strings [done, p.n) of a fixed-length batch through the generic kernel
int LaunchRemainder(const ScanParams& p, uint64_t done, hipStream_t stream);
int LaunchTiled(const ScanParams& p, hipStream_t stream);
// wide.hip: fixed-length records through the class-indexed walk (tables whose scans keep leaving the dense rows)
bool WideWanted(const ScanParams& p, const pire_hip_config& cfg);
int LaunchWide(const ScanParams& p, hipStream_t stream);
bool TiledEligible(const ScanParams& p);
bool RaggedEligible(const ScanParams& p, uint64_t totalBytesHint);
int LaunchRagged(const ScanParams& p, unsigned long long* workCounter, hipStream_t stream);
int LaunchRaggedWide(const ScanParams& p, unsigned long long* workCounter, hipStream_t stream);   // ... on the class-indexed walk
// stream.hip: offset batches of many short strings, every lane a run of consecutive strings
bool StreamEligible(const ScanParams& p, uint64_t totalBytesHint);
int LaunchStream(const ScanParams& p, hipStream_t stream);
bool StreamWideEligible(const ScanParams& p, uint64_t totalBytesHint);   // ... on the class-indexed walk (offset batches of a wide table)
int LaunchStreamWide(const ScanParams& p, hipStream_t stream);
// segmented.hip: few long strings, cut into segments that are scanned in parallel (speculatively; the chain of
// segments is then followed on the host, so the call synchronises its stream)
bool SegmentedEligible(uint64_t n, uint64_t totalBytes);
int RunSegmented(pire_hip_table* t, const ScanParams& p, const uint64_t* hostOffsets, hipStream_t stream,
                 uint32_t* halfFinalResults = nullptr,    // non-null: also HalfFinalScanner counts, [n][regexps] ...
                 bool* halfFinalIncomplete = nullptr);    // ... unless some string ended in the plain walk (then true)
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) and the occupancy query cost the host several microseconds per
// launch; what they say does not change: remembered per device and kernel (the LDS limit as a high-water mark).
struct LaunchCache {
	struct Key {
		int dev;
		const void* fn;
		int threads;
		uint32_t lds;
		bool operator==(const Key& o) const { return dev == o.dev && fn == o.fn && threads == o.threads && lds == o.lds; }
	};
	struct Entry {
		Key key;
		int value;
	};
	std::mutex mutex;
	std::vector<Entry> ldsMax, occupancy;
	static LaunchCache& Get()
	{
		static LaunchCache c;
		return c;
	}
};

inline hipError_t SetDynamicLds(const void* fn, uint32_t ldsBytes)
{
	int dev = 0;
	hipError_t e = hipGetDevice(&dev);
	if (e != hipSuccess)
		return e;
	LaunchCache& c = LaunchCache::Get();
	std::lock_guard<std::mutex> lock(c.mutex);
	LaunchCache::Entry* found = nullptr;
	for (auto& x : c.ldsMax)
		if (x.key.dev == dev && x.key.fn == fn)
			found = &x;
	if (found && uint32_t(found->value) >= ldsBytes)
		return hipSuccess;
	e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(ldsBytes));
	if (e != hipSuccess)
		return e;
	if (found)
		found->value = int(ldsBytes);
	else
		c.ldsMax.push_back({{dev, fn, 0, 0}, int(ldsBytes)});
	return hipSuccess;
}

// The launch of a kernel with dynamic LDS: the attribute (remembered above), the launch, its error as a return code.
template <class... A, class... P>
int Launch(void (*kernel)(A...), unsigned blocks, unsigned threads, uint32_t ldsBytes, hipStream_t stream, const char* what,
           const P&... args)
{
	hipError_t e = SetDynamicLds(reinterpret_cast<const void*>(kernel), ldsBytes);
	if (e != hipSuccess)
		return HipFail(e, "hipFuncSetAttribute(LDS)");
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), ldsBytes, stream, args...);
	e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, what);
}

// The CUs of the current device (*dev, where asked for).
inline int DeviceCUs(int* cus, int* dev = nullptr)
{
	// asked on every launch: cache per device (hipGetDeviceProperties is far too slow for that)
	static std::atomic<int> cached[64];
	int d = 0;
	hipError_t e = hipGetDevice(&d);
	if (e != hipSuccess)
		return HipFail(e, "hipGetDevice");
	const bool slot = d >= 0 && d < 64;
	int v = slot ? cached[d].load(std::memory_order_relaxed) : 0;
	if (v == 0) {
		e = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d);
		if (e != hipSuccess)
			return HipFail(e, "hipDeviceGetAttribute(multiprocessor count)");
		if (slot)
			cached[d].store(v, std::memory_order_relaxed);
	}
	*cus = v;
	if (dev)
		*dev = d;
	return PIRE_HIP_OK;
}

// Blocks of `threads` for n items, one per lane, of a kernel with `ldsBytes` of LDS: as many per CU as its 2048 threads
// and 160 KB allow, no more than the items fill.
inline unsigned GridBlocks(uint64_t n, int cus, unsigned threads, uint32_t ldsBytes)
{
	const uint64_t perCu = std::max<uint64_t>(1, std::min<uint64_t>(2048 / threads, (160 * 1024) / std::max<uint32_t>(ldsBytes, 1)));
	return unsigned(std::max<uint64_t>(1, std::min<uint64_t>((n + threads - 1) / threads, uint64_t(cus) * perCu)));
}

// The list a kernel with 16-bit state leaves the strings on that outgrow it: [0] = count (zeroed here, on the stream),
// then up to n string indices.
inline int OverflowList(StreamScratch& list, uint64_t n, hipStream_t stream, const char* what, uint32_t** out)
{
	if (int rc = list.Alloc((size_t(n) + 1) * 4, what))
		return rc;
	const hipError_t e = hipMemsetAsync(list.get(), 0, 4, stream);
	if (e != hipSuccess)
		return HipFail(e, what);
	*out = list.as<uint32_t>();
	return PIRE_HIP_OK;
}

// order.hip: the strings of an offset batch ordered by length class (longest first), built on the device, for the
// one-string-per-lane kernels with per-byte actions.
// The k of pass `pass` (k = pass * lanes + t, or the same range backwards in odd passes when `serpentine`), for the
// grid-stride loops of those kernels; >= n: nothing for this lane in this pass.
__host__ __device__ inline uint64_t OrderedIndex(uint64_t pass, uint64_t t, uint64_t lanes, bool serpentine)
{
	return pass * lanes + ((serpentine && (pass & 1)) ? lanes - 1 - t : t);
}
// Where the batch is large enough for it (and pire_hip_config.no_length_order is not set): builds the order in `scratch`
// -- the caller's owner, which has to live until the kernels that read *order are enqueued -- and says in *serpentine
// whether the kernels should walk it with OrderedIndex's serpentine (the global order) or plainly.  Else leaves both alone.
int OrderByLength(const uint64_t* offsets, uint64_t n, hipStream_t stream, StreamScratch& scratch, const uint32_t** order,
                  uint32_t* serpentine);
// Whether OrderByLength builds an order for a batch of n strings (for a launch plan that has to say so beforehand).
bool OrdersByLength(uint64_t n, const pire_hip_config& c);
// select.hip: from end states to matches (pire_hip_select).  UploadSelect: the mask image of the CURRENT device, built on
// first use (the caller holds t->adaptMutex, shared: the host image is built from t->host), copied out to *image (nullable).
// LaunchSelect: device pointers only, enqueues three small kernels on `stream`, scratch from the stream-ordered allocator.
uint32_t SelectMaskWords(uint32_t regexps);
int UploadSelect(pire_hip_table* t, SelectDevice* image);
void FreeSelect(pire_hip_table* t);
int LaunchSelect(const SelectDevice& image, uint32_t states, uint32_t words, const uint32_t* stateIdx, uint64_t n,
                 const uint64_t* want, uint64_t* outMasks, uint64_t* outHits, uint64_t* outHitMasks, uint64_t hitCap,
                 uint64_t* outHitCount, hipStream_t stream);
// The scan of every hit pass (select.hip, capture_select.hip, route.hip): exclusive scan of every row of
// counts[rows][entries] -- selected strings per tile of 1 024 -- in place, a block per row; outCounts[r] = the total of row r.
// Enqueues; the caller asks hipGetLastError() behind its launches.
void LaunchTileScan(uint32_t* counts, uint32_t rows, uint32_t entries, uint64_t* outCounts, hipStream_t stream);
// The front of every ballot compaction's launcher (tile_pass.h TilePass).  n == 0: *outHitCount is zeroed on the stream and
// s->tiles = 0 (nothing to launch); 2^32 strings or more: refused in `who`'s name; else s->tiles = ceil(n / 1024) and the one
// allocation of `scratch`, carved into s->ballots[tiles * 16] and s->tileCounts[tiles].
struct TileScratch;   // compact.h
int TileCompaction(const char* who, const char* scratchLabel, uint64_t n, uint64_t* outHitCount, hipStream_t stream, StreamScratch& scratch,
                   TileScratch* s);
// The count and the lists of a hit pass inside ONE call of an entry point, on whichever side the caller's pointers live: the
// one home of "the count comes back first; host pointers stage no list longer than min(hit_cap, n); the lists come back only
// as far as they were written".  Order: Count(), a List() for every list the pass writes (cap == 0 or a null array: no list,
// *dev = nullptr) -- the pass's other result arrays between them, where it has any --, io.Ready(), the launches on dCount,
// cap and the lists, io.Finish(), Back().  Device pointers pass through; Back() then does nothing.
struct HitStage {
	static constexpr uint32_t kMaxLists = 3;
	const bool onDevice;
	uint64_t* const outCount;    // the caller's
	const char* const backLabel; // names the copies back where one fails
	uint64_t cap = 0, count = 0; // host pointers: the count comes back in `count` first
	uint64_t* dCount = nullptr;
	struct Staged {
		void* host;
		const void* dev;
		size_t width;   // bytes an entry
	} lists[kMaxLists];
	uint32_t nLists = 0;
	HitStage(bool onDevice_, uint64_t* outCount_, const char* backLabel_) : onDevice(onDevice_), outCount(outCount_), backLabel(backLabel_) {}
	int Count(BatchIO& io, uint64_t hitCap, uint64_t n);   // n strings have at most n hits
	template <class T>
	int List(BatchIO& io, T* host, size_t perEntry, T** dev)   // perEntry elements of T an entry
	{
		*dev = nullptr;
		if (!host || !cap || !perEntry)
			return PIRE_HIP_OK;
		if (int rc = io.Result(host, size_t(cap) * perEntry, 0, dev))
			return rc;
		lists[nLists++] = Staged{host, *dev, perEntry * sizeof(T)};
		return PIRE_HIP_OK;
	}
	int Back();   // host pointers: the count to the caller, and every list as far as it was written
};
// capture_select.hip: from capture positions to a compacted, ascending list of byte ranges (pire_hip_capture_select).
// Device pointers only, three kernels enqueued on `stream`, scratch from the stream-ordered allocator.  fin == nullptr:
// Final is not asked for.  shift: string i lies shift * i bytes further into the buffer the spans are counted in (1: the
// offsets are pire_hip_split's and the spans are ranges of the raw buffer).
int LaunchCaptureSelect(const uint64_t* offsets, uint64_t n, bool beginMark, const long long* begin, const long long* end,
                        const uint8_t* fin, uint64_t shift, uint64_t* outHits, uint64_t* outSpans, uint64_t hitCap,
                        uint64_t* outHitCount, hipStream_t stream);
// What pire_hip_capture_select refuses of its outputs before any device is touched (haveList: the hits have somewhere to go)
int CaptureSelectOutputsInvalid(const char* who, uint64_t n, int needFinal, bool haveFinal, bool haveList, uint64_t hitCap,
                                const void* outHitCount);
// count_select.hip: from result rows to a compacted, ascending list of the strings whose counters reach their thresholds, and
// the occurrences of every regexp over the batch (pire_hip_count_select).  Device pointers only, three to four kernels
// enqueued on `stream`, scratch from the stream-ordered allocator: the compaction's, and regexps * ceil(n / 1024) * 8 bytes of
// tile sums where outTotals is not null.  n == 0 or regexps == 0: the count (and the totals) zeroed on the stream.
int LaunchCountSelect(const uint32_t* results, uint64_t n, uint32_t regexps, const uint32_t* minCount, uint32_t mode, uint64_t* outTotals,
                      uint64_t* outHits, uint32_t* outHitResults, uint64_t hitCap, uint64_t* outHitCount, hipStream_t stream);
// The pass's own arguments, as the caller of an entry point gave them
struct CountSelectOut {
	const uint32_t* minCount;
	uint32_t mode;
	uint64_t* outTotals;
	uint64_t* outHits;
	uint32_t* outHitResults;
	uint64_t hitCap;
	uint64_t* outHitCount;
};
// What pire_hip_count_select refuses before any device is touched, in `who`'s name (haveResults: there are rows to read)
int CountSelectArgsInvalid(const char* who, uint64_t n, uint32_t regexps, bool haveResults, const CountSelectOut& o);
// The pass inside ONE call of an entry point (pire_hip_count_select itself, and the scans it follows on their stream), on
// whichever side the caller's pointers live.  Order: Empty() instead of everything where there is nothing to read; else
// In() with the call's inputs, Results() with its result arrays, io.Ready(), the scan, Launch(), io.Finish(), Back().
struct CountSelectStage {
	const CountSelectOut o;
	const uint32_t regexps;
	HitStage list;   // the count, out_hits, out_hit_results
	const uint32_t* dMin = nullptr;
	uint64_t *dTotals = nullptr, *dHits = nullptr;
	uint32_t* dHitResults = nullptr;
	CountSelectStage(const CountSelectOut& o_, uint32_t regexps_, bool onDevice_)
		: o(o_), regexps(regexps_), list(onDevice_, o_.outHitCount, "hipMemcpy(hits)")
	{
	}
	int Empty(hipStream_t stream);   // no strings or no regexps: zeros -- host pointers: no device is touched
	int In(BatchIO& io);             // min_count
	int Results(BatchIO& io, uint64_t n);
	int Launch(const uint32_t* results, uint64_t n, hipStream_t stream);
	int Back() { return list.Back(); }
};
// counting.hip: pire_hip_counting_run, and behind it -- where sel is not null -- the pass above on the same stream, on the
// staged copy of a host-pointer call; outResults may then be null (the rows live in stream-ordered scratch).  `who` names the
// entry point in what is refused.
int CountingRunImpl(const char* who, pire_hip_counting_table* t, int kind, const void* text, const uint64_t* offsets, uint64_t n,
                    uint32_t flags, uint32_t* outIdx, uint32_t* outResults, const CountSelectOut* sel, hipStream_t stream);
// counting.hip: pire_hip_capture_run, and behind it -- where sel is not null -- the pass above on the same stream, on the
// staged copy of a host-pointer call.  The position and Final arrays the pass needs and the caller has no room for live in
// stream-ordered scratch.
struct CaptureSelectOut {
	int needFinal;
	uint64_t shift;
	uint64_t* outHits;
	uint64_t* outSpans;
	uint64_t hitCap;
	uint64_t* outHitCount;
};
int CaptureRunImpl(pire_hip_counting_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                   uint32_t* outIdx, uint8_t* outFinal, int64_t* outBegin, int64_t* outEnd, const CaptureSelectOut* sel,
                   hipStream_t stream);
// slow_capture.hip: pire_hip_slow_capture_run, and behind it -- where sel is not null -- the same pass with final = the captured
// flags; the result arrays may then be null.  `who` names the entry point in what is refused.
int SlowCaptureRunImpl(const char* who, pire_hip_slow_capture_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                       uint8_t* outCaptured, int64_t* outBegin, int64_t* outEnd, uint8_t* outMatched, const CaptureSelectOut* sel,
                       hipStream_t stream);
// slow_hits.hip: from Final flags to a compacted, ascending list of the strings whose flag is set -- or, with
// PIRE_HIP_FINAL_SELECT_ZERO, of those whose flag is not (pire_hip_final_select).  Device pointers only, three kernels enqueued
// on `stream`, the compaction's scratch from the stream-ordered allocator.  n == 0: the count zeroed on the stream.
int LaunchFinalSelect(const uint8_t* fin, uint64_t n, uint32_t mode, uint64_t* outHits, uint64_t hitCap, uint64_t* outHitCount,
                      hipStream_t stream);
// The pass's own arguments, as the caller of an entry point gave them
struct FinalSelectOut {
	uint32_t mode;
	uint64_t* outHits;
	uint64_t hitCap;
	uint64_t* outHitCount;
};
// What pire_hip_final_select refuses before any device is touched, in `who`'s name (haveFinal: there are flags to read)
int FinalSelectArgsInvalid(const char* who, uint64_t n, bool haveFinal, const FinalSelectOut& o);
// The pass inside ONE call of an entry point (pire_hip_final_select itself, and the slow scan it follows on its stream), on
// whichever side the caller's pointers live.  Order: Empty() instead of everything where there is nothing to read; else
// Results() with its result arrays, io.Ready(), the scan, Launch(), io.Finish(), Back().
struct FinalSelectStage {
	const FinalSelectOut o;
	HitStage list;   // the count, out_hits
	uint64_t* dHits = nullptr;
	FinalSelectStage(const FinalSelectOut& o_, bool onDevice_) : o(o_), list(onDevice_, o_.outHitCount, "hipMemcpy(hits)") {}
	int Empty(hipStream_t stream);   // no strings: a count of 0 -- host pointers: no device is touched
	int Results(BatchIO& io, uint64_t n);
	int Launch(const uint8_t* fin, uint64_t n, hipStream_t stream);
	int Back() { return list.Back(); }
};
// affix.hip: from prefix and suffix lengths to a compacted, ascending list of the strings that matched and the byte range of
// the matched head, the matched tail or what they leave (pire_hip_affix_select).  Device pointers only, three kernels enqueued
// on `stream`, the compaction's scratch from the stream-ordered allocator.  headLen / tailLen: nullable, not both where n > 0.
// shift: as LaunchCaptureSelect's.  n == 0: the count zeroed on the stream.
int LaunchAffixSelect(const uint64_t* offsets, uint64_t n, uint32_t part, const long long* headLen, const long long* tailLen,
                      uint64_t shift, uint64_t* outHits, uint64_t* outSpans, uint64_t hitCap, uint64_t* outHitCount, hipStream_t stream);
// The pass's own arguments, as the caller of an entry point gave them
struct AffixSelectOut {
	uint32_t part;
	uint64_t* outHits;
	uint64_t* outSpans;
	uint64_t hitCap;
	uint64_t* outHitCount;
};
// What pire_hip_affix_select refuses before any device is touched, in `who`'s name (have*: there is such an array to read;
// ownList: the entry point keeps the span list to itself where the caller has no array for it)
int AffixSelectArgsInvalid(const char* who, uint64_t n, bool haveOffsets, bool haveHead, bool haveTail, const AffixSelectOut& o,
                           bool ownList = false);
// The pass inside ONE call of an entry point (pire_hip_affix_select itself, and the two scans it follows on their stream), on
// whichever side the caller's pointers live.  Order: Empty() instead of everything where there is nothing to read; else
// Results() with its result arrays, io.Ready(), the scans, Launch(), io.Finish(), Back().
struct AffixSelectStage {
	const AffixSelectOut o;
	HitStage list;   // the count, out_hits, out_spans
	uint64_t *dHits = nullptr, *dSpans = nullptr;
	AffixSelectStage(const AffixSelectOut& o_, bool onDevice_) : o(o_), list(onDevice_, o_.outHitCount, "hipMemcpy(hits)") {}
	int Empty(hipStream_t stream);   // no strings: a count of 0 -- host pointers: no device is touched
	int Results(BatchIO& io, uint64_t n);
	int Launch(const uint64_t* offsets, uint64_t n, const int64_t* headLen, const int64_t* tailLen, hipStream_t stream);
	int Back() { return list.Back(); }
};
// context.hip: from an ascending hit list to the ascending list of the lines within `after` lines behind or `before` lines in
// front of a hit, and two bits a line (pire_hip_context).  Device pointers only -- hitCount included, nullable: k = hitCap --,
// three or four kernels enqueued on `stream`; scratch from the stream-ordered allocator: the compaction's and n / 4 bytes of
// hit and run words.  outLines == nullptr: counts only.  n == 0 or hitCap == 0: the counts zeroed on the stream.
int LaunchContext(const uint64_t* hits, const uint64_t* hitCount, uint64_t hitCap, uint64_t n, uint64_t before, uint64_t after,
                  uint64_t* outLines, uint8_t* outFlags, uint64_t lineCap, uint64_t* outLineCount, uint64_t* outGroupCount,
                  hipStream_t stream);
// The pass's own outputs, as the caller of an entry point gave them
struct ContextOut {
	uint64_t* outLines;
	uint8_t* outFlags;
	uint64_t lineCap;
	uint64_t* outLineCount;
	uint64_t* outGroupCount;
};
// What pire_hip_context refuses before any device is touched, in `who`'s name (haveHits: there is a list to read; ownList: the
// entry point keeps the line list to itself where the caller has no array for it)
int ContextArgsInvalid(const char* who, bool haveHits, uint64_t hitCap, uint64_t n, const ContextOut& o, bool ownList = false);
// What a host-pointer call refuses of its list: hits[0, k) -- any alignment -- strictly ascending, every entry < n
int ContextHitsInvalid(const char* who, const void* hits, uint64_t k, uint64_t n);
// combine.hip: from up to six ascending hit lists and a truth table over their member masks to the ascending list of the
// selected lines and the mask of each (pire_hip_combine).  Device pointers only -- the counts included, each nullable:
// k_j = caps[j] --, three kernels enqueued on `stream`; scratch from the stream-ordered allocator: the compaction's and,
// where outMembers is asked for, n bytes of member masks.  outHits == nullptr: the count only.  n == 0: the count zeroed on
// the stream.  The arrays of CombineLists are the host's and travel to the kernels by value.
struct CombineLists {
	const uint64_t* lists[PIRE_HIP_COMBINE_MAX_LISTS];
	const uint64_t* counts[PIRE_HIP_COMBINE_MAX_LISTS];
	uint64_t caps[PIRE_HIP_COMBINE_MAX_LISTS];
	uint32_t k;
};
int LaunchCombine(const CombineLists& in, uint64_t n, uint64_t truth, uint64_t* outHits, uint8_t* outMembers, uint64_t hitCap,
                  uint64_t* outHitCount, hipStream_t stream);
// The pass's own outputs, as the caller of an entry point gave them
struct CombineOut {
	uint64_t* outHits;
	uint8_t* outMembers;
	uint64_t hitCap;
	uint64_t* outHitCount;
};
// What pire_hip_combine refuses of its outputs and of n before any device is touched, in `who`'s name (ownList: the entry
// point keeps the list to itself where the caller has no array for it)
int CombineOutputsInvalid(const char* who, uint64_t n, const CombineOut& o, bool ownList = false);
// files.hip: from an ascending hit list and the files' line boundaries to hits by file (pire_hip_files).  Device pointers only
// -- hitCount included, nullable: k = hitCap --, four or five kernels enqueued on `stream`; scratch from the stream-ordered
// allocator: the compaction's over `files`, and the first row where outFileFirst is null.  outHits (nullable): the first
// min(k, outCap) entries of the list itself, for a caller whose list lives in scratch; outHitFile / outHitLine: outCap entries.
// files == 0: the count and outFileFirst[0] zeroed on the stream.
int LaunchFiles(const uint64_t* hits, const uint64_t* hitCount, uint64_t hitCap, const uint64_t* bounds, uint64_t files, uint32_t fileMode,
                uint64_t* outFileFirst, uint64_t* outHits, uint64_t* outHitFile, uint64_t* outHitLine, uint64_t outCap, uint64_t* outFiles,
                uint64_t fileCap, uint64_t* outFileCount, hipStream_t stream);
// outFileLines[f] for f in [0, files] = how many of the split's n lines (line i begins at offsets[i] + i of raw) begin in front
// of byte fileBytes[f]; *outStraddles = how many f in [1, files) have 0 < fileBytes[f] < size and raw[fileBytes[f] - 1] != delim.
// Two kernels, files / 256 bytes of scratch.
int LaunchFileLines(const uint64_t* offsets, uint64_t n, const uint64_t* fileBytes, uint64_t files, const void* raw, uint64_t size,
                    uint32_t delim, uint64_t* outFileLines, uint64_t* outStraddles, hipStream_t stream);
// The file list of the pass, as the caller of an entry point gave it
struct FilesOut {
	uint64_t* outFiles;
	uint64_t fileCap;
	uint64_t* outFileCount;
};
// What pire_hip_files and the lines forms refuse of the files before any device is touched, in `who`'s name (boundsName: what
// the entry point calls its boundaries), and what a host-pointer call refuses of the boundaries themselves: bounds[files + 1]
// non-decreasing from 0 to `total` (totalName: n or size)
int FilesArgsInvalid(const char* who, bool haveBounds, const char* boundsName, uint64_t files, uint32_t fileMode, const FilesOut& o);
int FilesBoundsInvalid(const char* who, const char* boundsName, const uint64_t* bounds, uint64_t files, uint64_t total, const char* totalName);
// split.hip: raw text into strings (pire_hip_split).  Device pointers only, everything enqueued on `stream`.  The pass
// comes in two halves because a caller may want the number of strings before it has room for their offsets:
// LaunchSplitCount counts and scans (*outN = n; the tile prefixes stay in `scratch`, the caller's owner, which has to live
// until the scatter is enqueued), LaunchSplitScatter writes offsets[0..min(n, cap)] and, where outText is not null, the text
// without its delimiters.  LaunchHitSpans: [begin, end) in the raw buffer of the first min(counts[r], kMax) hits of every row
// of hits[rows][pitch], spans[rows][pitch][2], one launch (one list: rows = 1, pitch = kMax = its capacity); `what` names
// the launch where it fails.
struct SplitPlan {
	const uint8_t* raw;
	uint32_t head;       // raw's address modulo 16: tiles and lanes are cut on the 16-byte grid, raw[0] is byte `head` of the first lane
	uint32_t delim4;     // the delimiter in every byte
	uint64_t size;
	uint32_t tiles;
	uint32_t* counts;    // [tiles] delimiters per tile
	uint64_t* prefix;    // [tiles] delimiters in front of the tile
};
int LaunchSplitCount(const void* raw, uint64_t size, uint32_t delim, uint64_t* outN, hipStream_t stream, StreamScratch& scratch,
                     SplitPlan* plan);
int LaunchSplitScatter(const SplitPlan& plan, void* outText, uint64_t* outOffsets, uint64_t offsetsCap, const uint64_t* outN,
                       hipStream_t stream);
int LaunchHitSpans(const uint64_t* hits, const uint64_t* counts, uint32_t rows, uint64_t pitch, uint64_t kMax, const uint64_t* offsets,
                   uint64_t* spans, hipStream_t stream, const char* what);
// route.hip: one ascending hit list per regexp (pire_hip_route).  Device pointers only, three kernels enqueued on `stream`,
// regexps * ceil(n / 1024) * 4 bytes of scratch from the stream-ordered allocator.  outHits[regexps][hitCap] (nullable:
// counts only), outHitCounts[regexps]; the image and the scan kernel are the select pass's.
int LaunchRoute(const SelectDevice& image, uint32_t states, uint32_t words, uint32_t regexps, const uint32_t* stateIdx, uint64_t n,
                uint64_t* outHits, uint64_t hitCap, uint64_t* outHitCounts, hipStream_t stream);
// gather.hip: the listed strings of a batch back to back (pire_hip_gather).  Device pointers only, four kernels enqueued on
// `stream`, no scratch and no allocation (outOffsets, cap + 1 entries, is required where cap > 0).  Where the source ranges come from:
// spans != nullptr -> raw[spans[2j], spans[2j + 1]) with raw = text and `size` its length; else offsets + idx (nullable:
// the identity) over n strings.  hostTotal: the total where the host knows it (it sizes the copy pass's grid exactly),
// kGatherTotalUnknown where it does not (the grid then comes from textCap, and blocks beyond *outBytes leave).
struct GatherSource {
	const uint8_t* text;
	const uint64_t* offsets;
	uint64_t n;
	const uint64_t* idx;
	const uint64_t* spans;
	uint64_t size;
};
constexpr uint64_t kGatherTotalUnknown = ~0ull;
int LaunchGather(const GatherSource& src, const uint64_t* count, uint64_t cap, uint32_t tail, void* outText, uint64_t textCap,
                 uint64_t* outOffsets, uint64_t* outBytes, uint64_t hostTotal, hipStream_t stream);
// fields.hip: where field `field` of every string is (pire_hip_fields).  Device pointers only, four kernels enqueued on
// `stream`, 16 bytes of scratch per block of the grid (<= 2 048) from the stream-ordered allocator.  bytesHint: an upper bound
// of offsets[n] - offsets[0] where the host knows one (it sizes the grid), kFieldsBytesUnknown where it does not (the grid is
// then the largest, and the blocks without a tile leave).
constexpr uint64_t kFieldsBytesUnknown = ~0ull;
int LaunchFields(const void* text, const uint64_t* offsets, uint64_t n, uint32_t sep, uint32_t field, uint32_t mode, uint64_t* outSpans,
                 uint64_t bytesHint, hipStream_t stream);
void NoteKernel(const char* name, const char* symbol = nullptr);   // what pire_hip_last_kernel[_symbol]() report (thread local)
bool RaggedActEligible(const ScanParams& p);
int LaunchRaggedHalfFinal(const ScanParams& p, unsigned long long* workCounter, uint32_t* outResults, hipStream_t stream);
// CapturingScanner on the ragged kernel with actions (counting.hip builds the table): `info` = per state of the
// EXPANDED automaton (reference numbering of that table): original state << 8 | Final tag << 2 | action that entered it
int LaunchRaggedCapture(const ScanParams& p, unsigned long long* workCounter, const uint32_t* info, long long* outBegin,
                        long long* outEnd, hipStream_t stream);
// api.cpp, for the other translation units: the scan parameters of a table on the current device (uploads the image,
// auto-adapts at the launch boundary), one ragged work slot of it, a table handle around a host table built elsewhere
// Holds a table still for ONE entry point: the automatic adaptation's turn first (no lock held), then the table's
// adaptMutex SHARED until the entry point returns, i.e. until its kernels are enqueued (host-pointer forms: until they
// have run).  pire_hip_table_adapt() and the automatic adaptation take the mutex exclusively, drain the devices and only
// then replace numbering and images -- so whatever an entry point derives from t->host after FillParams belongs to the
// image its ScanParams point at, and an adaptation may run concurrently with scans on other host threads (ADVICE r3:
// round 3 dropped the lock when FillParams returned).  Two tables (pire_hip_run_pair): acquire in address order.
extern thread_local const pire_hip_config* g_cfgOverride;   // api.cpp: what GetConfig() returns on this thread when set
// The table's own configuration (pire_hip_table_config_set), if it has one, as what GetConfig() returns on this thread while the
// scope lives: for an entry point, an adaptation (explicit, automatic or in the background worker), the ranking of a glued table
// and the entry self-tests, so that every GetConfig() on the paths that rank a table and build its images (ChooseZip,
// PermuteByScore, BuildDeviceImage, ScoreFromCounters) is the table's.  An override already in force stays: a first-use self-test
// in progress keeps its own (it already started from the table's).  Push(): the caller holds t->adaptMutex, shared or exclusive;
// the configuration is COPIED there, so the scope may outlive the lock.
struct TableConfigScope {
	pire_hip_config copy = {};
	const pire_hip_config* outer = nullptr;
	bool pushed = false;
	TableConfigScope() {}
	TableConfigScope(const TableConfigScope&) = delete;
	TableConfigScope& operator=(const TableConfigScope&) = delete;
	~TableConfigScope()
	{
		if (pushed)
			g_cfgOverride = outer;
	}
	void Push(const pire_hip_table* t)
	{
		if (pushed || !t->hasConfig || g_cfgOverride)
			return;
		copy = t->config;
		outer = g_cfgOverride;
		g_cfgOverride = &copy;
		pushed = true;
	}
};
struct TableUse {
	std::shared_lock<std::shared_mutex> lock;
	TableConfigScope cfg;
	TableUse() {}
	TableUse(pire_hip_table* t, bool enqueueOnly) { Acquire(t, enqueueOnly); }
	TableUse(const TableUse&) = delete;
	TableUse& operator=(const TableUse&) = delete;
	void Acquire(pire_hip_table* t, bool enqueueOnly)
	{
		if (lock.owns_lock())
			return;   // a second look at the same table inside one entry point (an adaptation would wait for this very lock)
		MaybeAutoAdapt(t, enqueueOnly);
		lock = std::shared_lock<std::shared_mutex>(t->adaptMutex);
		cfg.Push(t);   // for everything this entry point does on this thread
	}
};
// for the other translation units: TableUse::Acquire(t) + FillParams
int PrepareScanParams(pire_hip_table* t, ScanParams* p, uint32_t flags, TableUse* use, bool wantDist = false, bool enqueueOnly = false);
unsigned long long* TakeWorkSlot(pire_hip_table* t, const ScanParams& p);
void ChooseHotAndPermuteExported(HostTable& t);
int LaunchRaggedPrefix(const ScanParams& p, unsigned long long* workCounter, bool longest, bool throughEnd,
                       long long* outLen, hipStream_t stream);
int LaunchStep(const ScanParams& p, uint32_t* stateIdx, uint64_t n, uint32_t cls, hipStream_t stream);
int LaunchHalfFinal(const ScanParams& p, uint32_t* outResults, hipStream_t stream, unsigned long long* workCounter,
                    const uint32_t* list = nullptr);
// counting.hip: dense HalfFinal counting on the row kernel.  *done = false: not this table / batch.  Strings the 16-bit
// counters cannot hold are left on `*overflow` (device: [0] = count, then string indices; the caller's owner, allocated
// here) for LaunchHalfFinal(.., list).
int LaunchHalfFinalRows(pire_hip_table* t, const uint8_t* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                        uint32_t* outIdx, uint8_t* outFinal, uint32_t* outResults, hipStream_t stream, bool* done,
                        StreamScratch* overflow);
void FreeHalfRows(pire_hip_table* t);
int UploadHalfRows(pire_hip_table* t);   // counting.hip: the dense HalfFinal row image of the current device (first need / table_upload)
int LaunchPrefix(const ScanParams& p, bool longest, bool throughEnd, long long* outLen, hipStream_t stream,
                 unsigned long long* workCounter);
// pair.hip: two scanners in one pass over fixed-length records (run.h:229-241)
bool PairTiledEligible(const ScanParams& a, const ScanParams& b);
// the tiled kernel for the segmented scan's grid segments, warm-up inside the pass (tiled.hip, TiledSegParams)
int LaunchTiledSeg(const ScanParams& p, uint64_t warmBytes, const uint32_t* segJ, uint32_t* guess, hipStream_t stream);
// guessA != nullptr: the segmented scan's form (pair.hip, PairParams): warm-up inside the pass, the guesses written out
int LaunchPairTiled(const ScanParams& a, const ScanParams& b, uint32_t* outIdxB, hipStream_t stream, uint64_t warmBytes = 0,
                    const uint32_t* segJ = nullptr, uint32_t* guessA = nullptr, uint32_t* guessB = nullptr);
int LaunchOrFinal(uint8_t* fin, const uint8_t* other, uint64_t n, hipStream_t stream);
int LaunchSuffix(const ScanParams& p, bool longest, bool throughBegin, long long* outLen, hipStream_t stream);
// search.hip: the leftmost-longest match of every string (pire_hip_search), one launch: LongestSuffix through `rev`, then
// Longest- / ShortestPrefix through `fwd` from where it ended.  rev carries the batch (n, text, offsets: device pointers) and
// its start state (Initialize [+ EndMark]); fwd.startPerm is Initialize(), fwdStartBegin Initialize() + Step(BeginMark).
// opts: PIRE_HIP_SEARCH_*.  PIRE_HIP_EUNSUPPORTED before the launch where the two dense images do not fit a block's LDS.
int LaunchSearch(const ScanParams& rev, const ScanParams& fwd, uint32_t fwdStartBegin, uint32_t opts, long long* outBegin,
                 long long* outEnd, hipStream_t stream);
// search_all.hip: every leftmost-longest match of every string (pire_hip_search_all), four launches: the marks of one backward
// walk through `rev` and the matches per string, the scan of those into rows, the lists.  rev, fwd, fwdStartBegin, opts: as
// LaunchSearch.  textBytes: the buffer behind rev.text (offsets beyond it are clamped); shift: as LaunchCaptureSelect's.
// outRows[n + 1], outOwners[cap], outSpans[2 * cap]: nullable; *outCount: the matches, capped nowhere.  n == 0: the count
// (and outRows[0]) zeroed on the stream.
int LaunchSearchAll(const ScanParams& rev, const ScanParams& fwd, uint32_t fwdStartBegin, uint32_t opts, uint64_t textBytes, uint64_t shift,
                    uint64_t* outRows, uint64_t* outOwners, uint64_t* outSpans, uint64_t cap, uint64_t* outCount, hipStream_t stream);
// lex.hip: the matches of LaunchSearchAll with the regexps that accept each (pire_hip_lex), or -- PIRE_HIP_LEX_TOKENS -- the
// maximal-munch tokens of every string and the gaps between them, through `fwd` alone (`rev` is then not read).  Four launches
// either way: marks + counts (tokens: counts), the row scan of search_all.hip, the lists.  fwd carries the batch in token mode,
// rev otherwise, as LaunchSearchAll; fwd.acceptMaskPerm must be there.  outMasks[cap], outLabelCounts[fwd.regexps + 1]:
// nullable.  n == 0: the count, outRows[0] and the label counts zeroed on the stream.
int LaunchLex(const ScanParams& rev, const ScanParams& fwd, uint32_t fwdStartBegin, uint32_t opts, uint64_t textBytes, uint64_t shift,
              uint64_t* outRows, uint64_t* outOwners, uint64_t* outSpans, uint64_t* outMasks, uint64_t cap, uint64_t* outCount,
              uint64_t* outLabelCounts, hipStream_t stream);
// splice.hip: the spans of a buffer replaced by head ++ (the match, under PIRE_HIP_SPLICE_KEEP) ++ tail, the rest kept
// (pire_hip_splice).  Device pointers only -- but head and tail, which are the host's and travel as kernel arguments --, four
// kernels enqueued on `stream`, no allocation: outPos[cap] is required where cap > 0 (the caller's array or its scratch).
// offsets / outOffsets: nullable together.  hostTotal: *outBytes where the host knows it (it sizes the copy pass's grid
// exactly), kSpliceTotalUnknown where it does not (the grid then comes from textCap and the largest possible output).
constexpr uint64_t kSpliceTotalUnknown = ~0ull;
int LaunchSplice(const void* raw, uint64_t size, const uint64_t* spans, const uint64_t* count, uint64_t cap, const void* head, uint32_t headLen,
                 const void* tail, uint32_t tailLen, uint32_t mode, const uint64_t* offsets, uint64_t n, void* outText, uint64_t textCap,
                 uint64_t* outPos, uint64_t* outOffsets, uint64_t* outBytes, uint64_t hostTotal, hipStream_t stream);
int LaunchCorpusFill(uint8_t* out, uint64_t seed, uint64_t first, uint64_t count, uint64_t len, uint64_t stride,
                     const void* plantsHost, hipStream_t stream);

}  // namespace pirehip

