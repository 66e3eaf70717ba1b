// C ABI of libpire_hip.so (include/pire_hip.h).  Thin: argument checks, host<->device staging for the
// host-pointer convenience mode, kernel selection.  There is deliberately no CPU implementation of the walk
// here: without a HIP device the run entry points fail with PIRE_HIP_ENODEVICE.

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include <cerrno>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <new>
#include <stdexcept>

#include "internal.h"
#include "selftest.h"

namespace pirehip {

namespace {
thread_local std::string g_error;
thread_local const char* g_lastKernel = "none";
thread_local const char* g_lastSymbol = nullptr;
thread_local bool g_timing = false;
thread_local float g_lastMs = -1.0f;
}  // namespace

void SetError(const std::string& msg) { g_error = msg; }

// ---- device staging blocks cached between host-pointer calls (internal.h Staging) -------------------------------------
// Round 2 allocated and freed four or five device buffers in every host-pointer call of the prefix / suffix /
// half-final / counting / capture / slow entry points (77-110 us for 10 strings, most of it hipMalloc + hipFree, which
// also synchronise the device).  Blocks now come from per-device free lists by power-of-two size class and go back when
// the call returns (it has drained its stream by then); at most kStagingCacheBytes stay cached per device.
namespace {
constexpr size_t kStagingCacheBytes = size_t(1) << 30;
struct StagingCache {
	std::mutex mutex;
	std::vector<void*> free[48];   // by log2 of the block size
	size_t cached = 0;
};
StagingCache g_stagingCache[kMaxDevices];
int SizeClass(size_t bytes)
{
	int c = 12;   // 4 KiB at least
	while ((size_t(1) << c) < bytes)
		++c;
	return c;
}
}  // namespace

int StagingAcquire(size_t bytes, void** out, size_t* blockBytes)
{
	*out = nullptr;
	int dev = -1;
	hipError_t e = hipGetDevice(&dev);
	if (e != hipSuccess || dev < 0 || dev >= kMaxDevices)
		return HipFail(e == hipSuccess ? hipErrorInvalidDevice : e, "hipGetDevice");
	const int c = SizeClass(bytes);
	*blockBytes = size_t(1) << c;
	{
		StagingCache& cache = g_stagingCache[dev];
		std::lock_guard<std::mutex> lock(cache.mutex);
		if (!cache.free[c].empty()) {
			*out = cache.free[c].back();
			cache.free[c].pop_back();
			cache.cached -= *blockBytes;
			return PIRE_HIP_OK;
		}
	}
	e = hipMalloc(out, *blockBytes);
	if (e != hipSuccess)
		return HipFail(e, "hipMalloc(staging)");
	return PIRE_HIP_OK;
}

namespace {
StagingCache g_pinnedCache;   // host blocks are not per device
}
int StagingAcquireHost(size_t bytes, void** out, size_t* blockBytes)
{
	*out = nullptr;
	const int c = SizeClass(bytes);
	*blockBytes = size_t(1) << c;
	{
		std::lock_guard<std::mutex> lock(g_pinnedCache.mutex);
		if (!g_pinnedCache.free[c].empty()) {
			*out = g_pinnedCache.free[c].back();
			g_pinnedCache.free[c].pop_back();
			g_pinnedCache.cached -= *blockBytes;
			return PIRE_HIP_OK;
		}
	}
	const hipError_t e = hipHostMalloc(out, *blockBytes, hipHostMallocDefault);
	if (e != hipSuccess)
		return HipFail(e, "hipHostMalloc(staging)");
	return PIRE_HIP_OK;
}

void StagingReleaseHost(void* p, size_t blockBytes)
{
	{
		std::lock_guard<std::mutex> lock(g_pinnedCache.mutex);
		if (g_pinnedCache.cached + blockBytes <= (size_t(64) << 20)) {
			g_pinnedCache.free[SizeClass(blockBytes)].push_back(p);
			g_pinnedCache.cached += blockBytes;
			return;
		}
	}
	(void)hipHostFree(p);
}

void StagingRelease(void* p, size_t blockBytes)
{
	int dev = -1;
	if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxDevices) {
		StagingCache& cache = g_stagingCache[dev];
		std::lock_guard<std::mutex> lock(cache.mutex);
		if (cache.cached + blockBytes <= kStagingCacheBytes) {
			cache.free[SizeClass(blockBytes)].push_back(p);
			cache.cached += blockBytes;
			return;
		}
	}
	(void)hipFree(p);
}

int HandleException() noexcept
{
	try {
		try {
			throw;
		} catch (const std::bad_alloc&) {
			g_error = "out of memory";
			return PIRE_HIP_ENOMEM;
		} catch (const std::length_error&) {
			g_error = "out of memory (a table of that size cannot be built)";
			return PIRE_HIP_ENOMEM;
		} catch (const std::exception& e) {
			g_error = std::string("internal error: ") + e.what();
			return PIRE_HIP_EINVAL;
		} catch (...) {
			g_error = "internal error";
			return PIRE_HIP_EINVAL;
		}
	} catch (...) {   // building the message failed too
		return PIRE_HIP_ENOMEM;
	}
}

int HipFail(hipError_t e, const char* what)
{
	g_error = std::string(what) + ": " + hipGetErrorString(e);
	(void)hipGetLastError();   // clear the sticky error
	return e == hipErrorOutOfMemory ? PIRE_HIP_ENOMEM : PIRE_HIP_ENODEVICE;
}

namespace {


// The caller holds the table's TableUse (internal.h): no adaptation between here and the caller's return.
// wantDist: also the image's per-state distance tables (EnsureActDist).
int FillParams(pire_hip_table* t, ScanParams* p, uint32_t flags, bool wantDist = false)
{
	DeviceTable d;   // a copy of the current device's image (pointers), taken under the table's lock
	if (int rc = UploadTable(t, &d))
		return rc;
	const HostTable& h = t->host;
	memset(p, 0, sizeof(*p));
	p->workBase = d.workCounter;
	p->workDevice = d.device >= 0 && d.device < kMaxDevices ? d.device : 0;
	p->hotRows = d.hotRows;
	p->hotRowsRot = d.hotRowsRot;
	p->topShare = h.topShare;
	p->hotFlags = d.hotFlags;
	p->cls = d.cls;
	p->nextPerm = d.nextPerm;
	p->flagsPerm = d.flagsPerm;
	p->origOfPerm = d.origOfPerm;
	p->permOfOrig = d.permOfOrig;
	p->acceptMaskPerm = d.acceptMaskPerm;
	p->acceptOffPerm = d.acceptOffPerm;
	p->acceptIds = d.acceptIds;
	p->finSelf = d.finSelf;
	p->finEnd = d.finEnd;
	p->visitHot = d.visitHot;
	p->visitCold = d.visitCold;
	p->trapSignal = d.trapSignalDev;
	p->compactRows = d.compactRows;
	p->compact = h.compact;
	p->wideRows = d.wideRows;
	p->next16 = d.next16;
	p->visitWide = d.visitWide;
	p->wide = d.wideRows ? h.wide : 0;
	p->zipFull = d.wideRows ? h.zipFull : 0;
	p->wideOutSlot = p->wide;
	p->wideRowsStream = d.wideRows ? d.wideRowsStream : nullptr;
	p->wideStream = d.wideRows ? d.wideStream : 0;
	p->outsideDense = h.outsideDense;
	p->outsideWide = h.outsideWide;
	p->massMeasured = h.massMeasured;
	if (!h.massMeasured && d.trapSignalHost) {
		// A table nobody has adapted yet: what its scans so far left in the trap signal (mapped host memory: a read) says more
		// about the share of the steps outside the dense rows than the a-priori byte model -- a sampled trap stands for 1 024
		// lane-steps there.  The choice of the walk (WideWanted) follows it from the launch after the first ones have run.
		const uint64_t bytes = t->bytesScanned.load(std::memory_order_relaxed);
		const uint64_t traps = *d.trapSignalHost;
		if (bytes >= (uint64_t(1) << 22) && traps >= 64) {
			const float live = float(std::min(1.0, double(traps) * 1024.0 / double(bytes)));
			if (live > p->outsideDense) {
				p->outsideDense = live;
				p->massMeasured = true;
			}
		}
	}
	p->wideLaunched = &t->wideLaunched;
	p->incPerm = d.incPerm;
	p->hotFinalLo = h.hotFinalLo;
	p->hotDeadLo = h.hotDeadLo;
	p->deadShare = h.deadShare;
	p->finalShare = h.finalShare;
	p->states = h.states;
	p->letters = h.letters;
	p->regexps = h.regexps;
	p->hot = h.hot;
	p->beginCls = h.cls[kBeginMark];
	p->endCls = h.cls[kEndMark];
	p->flags = flags;
	uint32_t start = h.initial;                                     // Initialize(), multi.h:161
	if (flags & PIRE_HIP_RUN_BEGIN)
		start = h.next[size_t(start) * h.letters + h.cls[kBeginMark]];  // Begin(), run.h:375
	p->startPerm = h.permOfOrig[start];
	p->hostPermOfOrig = h.permOfOrig.data();
	p->hostOrigOfPerm = h.origOfPerm.data();
	p->owner = t;
	if (wantDist)
		if (int rc = EnsureActDist(t, &p->distFinalPerm, &p->distFlaggedPerm))
			return rc;
	return PIRE_HIP_OK;
}

}  // namespace
// ---- library configuration (pire_hip_config) ----------------------------------------------------------------------------
namespace {
std::mutex g_cfgMutex;

uint64_t EnvU64(const char* name)
{
	const char* v = getenv(name);
	if (!v || !*v)
		return 0;
	char* end = nullptr;
	const unsigned long long x = strtoull(v, &end, 10);
	return end != v ? uint64_t(x) : 1;   // PIRE_HIP_NO_SEGMENTS=yes counts as set
}

// The environment seeds the defaults ONCE (static initialisation of the first GetConfig / config_set call).
pire_hip_config SeedFromEnvironment()
{
	pire_hip_config c;
	memset(&c, 0, sizeof(c));
	c.size = sizeof(c);
	c.tiled_variant = uint32_t(EnvU64("PIRE_HIP_TILED_VARIANT"));
	c.checked = EnvU64("PIRE_HIP_CHECKED") == 1;
	c.no_compact = EnvU64("PIRE_HIP_NO_COMPACT") != 0;
	c.prior_flat = EnvU64("PIRE_HIP_PRIOR_FLAT") != 0;
	c.ragged_act_always = EnvU64("PIRE_HIP_RAGGED_ACT_ALWAYS") != 0;
	c.no_ragged_act = EnvU64("PIRE_HIP_NO_RAGGED_ACT") != 0;
	c.no_segments = EnvU64("PIRE_HIP_NO_SEGMENTS") != 0;
	c.segment_no_grid = EnvU64("PIRE_HIP_SEGMENT_NO_GRID") != 0;
	c.segment_stats = EnvU64("PIRE_HIP_SEGMENT_STATS") != 0;
	c.segment_modes = uint32_t(EnvU64("PIRE_HIP_SEGMENT_MODES"));
	c.segment_bytes = EnvU64("PIRE_HIP_SEGMENT_BYTES");
	if (getenv("PIRE_HIP_SEGMENT_WARMUP"))
		c.segment_warmup = EnvU64("PIRE_HIP_SEGMENT_WARMUP") ? EnvU64("PIRE_HIP_SEGMENT_WARMUP") : PIRE_HIP_SEGMENT_WARMUP_NONE;
	if (getenv("PIRE_HIP_SEGMENT_BUDGET"))
		c.segment_budget = EnvU64("PIRE_HIP_SEGMENT_BUDGET") ? EnvU64("PIRE_HIP_SEGMENT_BUDGET") : PIRE_HIP_SEGMENT_BUDGET_NONE;
	c.host_chunk_bytes = EnvU64("PIRE_HIP_HOST_CHUNK_BYTES");
	c.host_one_shot = EnvU64("PIRE_HIP_HOST_ONE_SHOT") != 0;
	c.no_rccl = EnvU64("PIRE_HIP_NO_RCCL") != 0;
	c.slow_sets_in_memory = EnvU64("PIRE_HIP_SLOW_SETS_IN_MEMORY") == 1;
	c.slow_no_list = EnvU64("PIRE_HIP_SLOW_NO_LIST") != 0;
	c.auto_adapt = uint32_t(EnvU64("PIRE_HIP_AUTO_ADAPT"));
	c.auto_adapt_min_traps = uint32_t(EnvU64("PIRE_HIP_AUTO_ADAPT_MIN_TRAPS"));
	c.ragged_variant = uint32_t(EnvU64("PIRE_HIP_RAGGED_VARIANT"));
	c.host_staging = uint32_t(EnvU64("PIRE_HIP_HOST_STAGING"));
	c.no_offsets_peek = EnvU64("PIRE_HIP_NO_OFFSETS_PEEK") != 0;
	c.segment_no_pair = EnvU64("PIRE_HIP_SEGMENT_NO_PAIR") != 0;
	c.segment_no_product = EnvU64("PIRE_HIP_SEGMENT_NO_PRODUCT") != 0;
	c.segment_no_derive = EnvU64("PIRE_HIP_SEGMENT_NO_DERIVE") != 0;
	c.no_length_order = EnvU64("PIRE_HIP_NO_LENGTH_ORDER") != 0;
	c.capture_by_length = EnvU64("PIRE_HIP_CAPTURE_BY_LENGTH") != 0;
	c.force_rccl = EnvU64("PIRE_HIP_FORCE_RCCL") != 0;
	c.counting_variant = uint32_t(EnvU64("PIRE_HIP_COUNTING_VARIANT"));
	c.slow_stats = EnvU64("PIRE_HIP_SLOW_STATS") != 0;
	c.walk_variant = uint32_t(EnvU64("PIRE_HIP_WALK_VARIANT"));
	c.selftest = uint32_t(EnvU64("PIRE_HIP_SELFTEST"));
	c.zip_variant = uint32_t(EnvU64("PIRE_HIP_ZIP_VARIANT"));
	return c;
}

pire_hip_config& ConfigStorage()
{
	static pire_hip_config c = SeedFromEnvironment();
	return c;
}
}  // namespace

thread_local const pire_hip_config* g_cfgOverride = nullptr;
thread_local bool g_inEntrySelfTest = false;

pire_hip_config GetConfig()
{
	if (g_cfgOverride)
		return *g_cfgOverride;   // a first-use self-test on this thread (selftest.h): its routing knobs
	std::lock_guard<std::mutex> lock(g_cfgMutex);
	return ConfigStorage();
}

int RunKnownAnswer(const std::vector<ConfigEdit>& edits, const std::function<void()>& poison,
                   const std::function<int(hipStream_t)>& call, const std::function<int()>& compare)
{
	OwnStream own;
	const pire_hip_config base = GetConfig();
	const pire_hip_config* const outer = g_cfgOverride;
	const bool was = g_inEntrySelfTest;
	int rc = PIRE_HIP_OK;
	for (size_t k = 0; k < edits.size() && rc == PIRE_HIP_OK; ++k) {
		pire_hip_config c = base;
		c.auto_adapt = 1;      // the table is not re-ranked under a self-test
		c.selftest = 1;        // ... and what the variant's call dispatches to is not tested again from inside
		c.no_segments = 1;
		edits[k](c);
		g_cfgOverride = &c;
		g_inEntrySelfTest = true;
		try {
			poison();
			rc = call(own.s);
			if (rc == PIRE_HIP_OK)
				rc = compare();
		} catch (...) {
			g_cfgOverride = outer;
			g_inEntrySelfTest = was;
			throw;
		}
		if (rc == PIRE_HIP_OK)
			NoteSelfTested(pire_hip_last_kernel());
		g_cfgOverride = outer;
		g_inEntrySelfTest = was;
	}
	return rc;
}

int SelfTestMismatch(const char* what, uint32_t string, const std::string& got, const std::string& want)
{
	SetError(std::string("self-test of ") + what + " (kernel '" + pire_hip_last_kernel() + "') failed: string " + std::to_string(string) +
	         " of the known-answer batch gave " + got + ", the table's transitions give " + want + " -- this build of libpire_hip.so (" +
	         pire_hip_build_info() + ") must not be used on this device");
	return PIRE_HIP_ESELFTEST;
}

bool EntrySelfTestDue(hipStream_t stream, uint32_t* mode)
{
	if (g_inEntrySelfTest)
		return false;
	*mode = GetConfig().selftest;
	if (*mode == 1)
		return false;
	hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
	return hipStreamIsCapturing(stream, &capturing) != hipSuccess || capturing == hipStreamCaptureStatusNone;
}

namespace {
std::mutex g_testedMutex;
std::string g_tested;   // ",name,name,"
}  // namespace

void NoteSelfTested(const char* kernel)
{
	std::lock_guard<std::mutex> lock(g_testedMutex);
	const std::string key = std::string(",") + kernel + ",";
	if (g_tested.empty())
		g_tested = ",";
	if (g_tested.find(key) == std::string::npos)
		g_tested += std::string(kernel) + ",";
}

std::string SelfTestedKernels()
{
	std::lock_guard<std::mutex> lock(g_testedMutex);
	return g_tested;
}

void NoteKernel(const char* name, const char* symbol)
{
	g_lastKernel = name;
	g_lastSymbol = symbol;
}
namespace {

// One slot of the table's ring of ragged work counters per launch (launches of one table may overlap on streams).
unsigned long long* NextWorkSlot(pire_hip_table* t, const ScanParams& p)
{
	return WorkSlotOf(p.workBase, t->workSlot[p.workDevice].fetch_add(1));
}

}  // namespace
int PrepareScanParams(pire_hip_table* t, ScanParams* p, uint32_t flags, TableUse* use, bool wantDist, bool enqueueOnly)
{
	use->Acquire(t, enqueueOnly);
	return FillParams(t, p, flags, wantDist);
}
unsigned long long* TakeWorkSlot(pire_hip_table* t, const ScanParams& p) { return NextWorkSlot(t, p); }
namespace {

// ---- first-use self-test (pire_hip_config.selftest) ---------------------------------------------------------------------
// The kernels below keep text on its way in registers and count their own waits; the build argues from the ISA that this
// is sound (tools/audit), this checks it where it runs: the first time a table takes one of Dispatch's kernels, that
// kernel scans a batch whose answer the host image's transitions give (the accessor walk of pire_hip_table_next, 131 072
// steps), on a stream and with visit counters of its own.  The text is a walk through the table's own states that
// stays out of the dead ones where it can, so that the end state depends on every byte of the string.
enum KernelKind : int { kKindGeneric, kKindTiled, kKindWide, kKindRagged, kKindRaggedWide, kKindStream, kKindStreamWide };

int SelfTest(const ScanParams& p, int kind, const char* name, uint32_t mode)
{
	constexpr uint32_t kStrings = 256, kLen = 512;
	const HostTable& h = p.owner->host;
	std::vector<uint8_t> text(size_t(kStrings) * kLen);
	std::vector<uint32_t> want(kStrings);
	std::vector<uint64_t> offsets(kStrings + 1);
	uint64_t rng = 0x9E3779B97F4A7C15ull ^ (uint64_t(h.states) << 20) ^ h.letters;
	auto next = [&](uint32_t st, uint32_t ch) { return h.next[size_t(st) * h.letters + h.cls[ch]]; };
	const uint32_t start = p.hostOrigOfPerm[p.startPerm];
	for (uint32_t i = 0; i < kStrings; ++i) {
		uint32_t st = start;
		offsets[i] = uint64_t(i) * kLen;
		for (uint32_t j = 0; j < kLen; ++j) {
			uint32_t ch = 0, to = st;
			for (int attempt = 0; attempt < 4; ++attempt) {
				rng = rng * 6364136223846793005ull + 1442695040888963407ull;
				// (printable text twice out of three times: what the tables here are mostly about)
				ch = (rng >> 33) % 3 ? 32 + uint32_t(rng >> 40) % 95 : uint32_t(rng >> 40) & 255;
				to = next(st, ch);
				if (!(h.flags[to] & kDead))
					break;
			}
			text[size_t(i) * kLen + j] = uint8_t(ch);
			st = to;
		}
		if (p.flags & PIRE_HIP_RUN_END)
			st = next(st, kEndMark);
		want[i] = st;
	}
	offsets[kStrings] = uint64_t(kStrings) * kLen;
	if (mode == 2)
		want[kStrings / 2] ^= 1;   // tests of the failure path
	// one block: text | offsets | end states | work counter | visit counters (dense rows, wide rows, every state)
	const size_t offOffsets = text.size(), offOut = offOffsets + offsets.size() * 8, offWork = offOut + kStrings * 4;
	const size_t offHot = offWork + 256, offWide = offHot + kVisitHotSlots * 4;
	const size_t offCold = offWide + (size_t(p.wide) + 1) * 4, bytes = offCold + size_t(p.states) * 4;
	void* block = nullptr;
	size_t blockBytes = 0;
	if (int rc = StagingAcquire(bytes, &block, &blockBytes))
		return rc;
	uint8_t* base = static_cast<uint8_t*>(block);
	hipStream_t own = nullptr;
	hipError_t e = hipStreamCreateWithFlags(&own, hipStreamNonBlocking);
	std::vector<uint32_t> got(kStrings, ~0u);
	int rc = PIRE_HIP_OK;
	const int passes = kind == kKindWide ? 2 : 1;   // the class-indexed walk: with one and with two strings per lane
	for (int pass = 0; pass < passes && e == hipSuccess && rc == PIRE_HIP_OK; ++pass) {
		if ((e = hipMemsetAsync(base + offOut, 0xFF, bytes - offOut, own)) != hipSuccess ||
		    (e = hipMemsetAsync(base + offWork, 0, bytes - offWork, own)) != hipSuccess ||
		    (e = hipMemcpyAsync(base, text.data(), text.size(), hipMemcpyHostToDevice, own)) != hipSuccess ||
		    (e = hipMemcpyAsync(base + offOffsets, offsets.data(), offsets.size() * 8, hipMemcpyHostToDevice, own)) != hipSuccess)
			break;
		std::atomic<uint64_t> launched{0};
		ScanParams q = p;
		q.text = base;
		q.textEnd = text.size();
		q.ends = nullptr;
		q.initIdx = nullptr;
		q.outIdx = reinterpret_cast<uint32_t*>(base + offOut);
		q.outFinal = nullptr;
		q.outCounts = nullptr;
		q.flags = p.flags & (PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END);
		q.n = kStrings;
		q.len = kLen;
		q.stride = kLen;
		q.offsets = kind == kKindTiled || kind == kKindWide ? nullptr : reinterpret_cast<const uint64_t*>(base + offOffsets);
		q.visitHot = reinterpret_cast<uint32_t*>(base + offHot);
		q.visitWide = reinterpret_cast<uint32_t*>(base + offWide);
		q.visitCold = reinterpret_cast<uint32_t*>(base + offCold);
		q.trapSignal = nullptr;
		q.wideLaunched = &launched;
		q.forceLanes = pass ? 2 : 1;   // (the batch is too small for LaunchWide to choose two strings per lane by itself)
		unsigned long long* work = reinterpret_cast<unsigned long long*>(base + offWork);
		rc = kind == kKindWide ? LaunchWide(q, own) : kind == kKindTiled ? LaunchTiled(q, own)
		     : kind == kKindRaggedWide ? LaunchRaggedWide(q, work, own) : kind == kKindStream ? LaunchStream(q, own)
		     : kind == kKindStreamWide ? LaunchStreamWide(q, own) : kind == kKindRagged ? LaunchRagged(q, work, own) : LaunchGeneric(q, own);
		if (rc != PIRE_HIP_OK)
			break;
		if ((e = hipMemcpyAsync(got.data(), base + offOut, kStrings * 4, hipMemcpyDeviceToHost, own)) != hipSuccess ||
		    (e = hipStreamSynchronize(own)) != hipSuccess)
			break;
		for (uint32_t i = 0; i < kStrings; ++i)
			if (got[i] != want[i]) {
				SetError(std::string("self-test of the ") + name + " kernel failed: string " + std::to_string(i) + " of the known-answer batch ended in state " +
				         std::to_string(got[i]) + ", the table's transitions give " + std::to_string(want[i]) +
				         " -- this build of libpire_hip.so (" + pire_hip_build_info() + ") must not be used on this device");
				rc = PIRE_HIP_ESELFTEST;
				break;
			}
	}
	if (own) {
		// (an error path may leave the kernel or a copy on its way: the block goes back to the cache only behind them -- ADVICE r5)
		(void)hipStreamSynchronize(own);
		(void)hipStreamDestroy(own);
	}
	StagingRelease(block, blockBytes);
	if (rc == PIRE_HIP_OK && e != hipSuccess)
		rc = HipFail(e, "self-test");
	return rc;
}

int Dispatch(const ScanParams& p, hipStream_t stream, unsigned long long* workCounter = nullptr,
             uint64_t totalBytesHint = 0)
{
	if (p.n == 0)
		return PIRE_HIP_OK;
	const bool tiled = !(p.flags & PIRE_HIP_RUN_GENERIC) && TiledEligible(p);
	const bool ragged = !tiled && !(p.flags & PIRE_HIP_RUN_GENERIC) && workCounter && RaggedEligible(p, totalBytesHint);
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	if (g_timing) {
		if (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)
			return HipFail(hipGetLastError(), "hipEventCreate");
		(void)hipEventRecord(ev0, stream);
	}
	// a table whose scans keep leaving the dense rows: the class-indexed walk (wide.hip; offset batches: the ragged kernel on it)
	const bool wideTable = (tiled || ragged) && WideWanted(p, GetConfig());
	const bool wide = tiled && p.len >= 256 && wideTable;
	const bool streamWide = ragged && wideTable && StreamWideEligible(p, totalBytesHint);
	const bool raggedWide = ragged && wideTable && !streamWide;
	const bool streamed = ragged && !wideTable && StreamEligible(p, totalBytesHint);
	const int kind = wide ? kKindWide : tiled ? kKindTiled : streamWide ? kKindStreamWide : raggedWide ? kKindRaggedWide : streamed ? kKindStream
	                 : ragged ? kKindRagged : kKindGeneric;
	static const char* const kNames[] = {"generic", "tiled", "wide", "ragged", "ragged_wide", "stream", "stream_wide"};
	static_assert(kSelfTestedOnWideImage == ((1u << kKindWide) | (1u << kKindRaggedWide) | (1u << kKindStreamWide) | (0xFu << 8)),
	              "internal.h kSelfTestedOnWideImage: the kinds on the wide image and the entry bits");
	if (p.owner && !(p.owner->selfTested[p.workDevice].load(std::memory_order_relaxed) & (1u << kind))) {
		const uint32_t mode = GetConfig().selftest;
		hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
		if (mode != 1 && !(p.flags & (1u << 23)) &&   // (bit 23: device_common.h kPermIds, the segmented scan's internal passes)
		     (hipStreamIsCapturing(stream, &capturing) != hipSuccess || capturing == hipStreamCaptureStatusNone)) {
			if (int rc = SelfTest(p, kind, kNames[kind], mode)) {
				if (ev0)
					(void)hipEventDestroy(ev0);
				if (ev1)
					(void)hipEventDestroy(ev1);
				return rc;
			}
			p.owner->selfTested[p.workDevice].fetch_or(1u << kind);
			NoteSelfTested(kNames[kind]);
		}
	}
	NoteKernel(kNames[kind]);
	if (p.owner && !(p.flags & (1u << 23)))   // (what the live estimate of FillParams divides the trap signal by)
	{
		// (offsets on the device: the host does not know the bytes -- the hint is ~0, which round 6's first form ADDED to the count:
		// it wrapped.  What the live estimate of FillParams divides by takes nothing for such a batch -- a guess there would turn
		// tables to the other walk on a guess --; the share of offset batches takes 48 bytes a string.)
		const bool known = !p.offsets || totalBytesHint != ~0ull;
		const uint64_t bytes = !p.offsets ? p.n * p.len : known ? totalBytesHint : p.n * 48;
		if (known)
			p.owner->bytesScanned.fetch_add(bytes, std::memory_order_relaxed);
		p.owner->bytesNominal.fetch_add(bytes, std::memory_order_relaxed);
		if (p.offsets)
			p.owner->bytesOffsetBatches.fetch_add(bytes, std::memory_order_relaxed);
	}
	int rc = wide ? LaunchWide(p, stream) : tiled ? LaunchTiled(p, stream) : streamWide ? LaunchStreamWide(p, stream)
	         : raggedWide ? LaunchRaggedWide(p, workCounter, stream) : streamed ? LaunchStream(p, stream)
	         : ragged ? LaunchRagged(p, workCounter, stream) : LaunchGeneric(p, stream);
	if (g_timing) {
		(void)hipEventRecord(ev1, stream);
		if (rc == PIRE_HIP_OK) {
			hipError_t e = hipEventSynchronize(ev1);
			if (e != hipSuccess)
				rc = HipFail(e, "hipEventSynchronize");
			else
				(void)hipEventElapsedTime(&g_lastMs, ev0, ev1);
		}
		(void)hipEventDestroy(ev0);
		(void)hipEventDestroy(ev1);
	}
	return rc;
}

// ---- host-pointer mode, chunked ---------------------------------------------------------------------------------------
// The batch is cut into chunks of whole strings (up to kHostChunkBytes of text each).  Chunk k goes
//     H2D text (+ its offsets / resume states)  ->  scan  ->  D2H results (into pinned staging)
// on stream k % 2 of a staging arena, so that the transfer of chunk k+1 overlaps the scan and the result copies of
// chunk k, the device staging is bounded whatever the batch size, and nothing is allocated per call: arenas (two
// streams, two sets of buffers grown on demand) are pooled per device for the life of the process.
// Measured (profiles/r02_pcie_probe.log, r02_host_mode.log): a scan is ~1 % of its own transfer, so the overlap buys
// little; what matters is (a) no hipMalloc/hipFree per call, (b) results never copied device -> PAGEABLE host inside
// the loop (that call blocks until the chunk's scan is over and serialises everything), (c) LARGE chunks -- the
// runtime stages pageable memory faster in few big copies (53 GB/s for 1 GiB at once, 47 in 32 MiB pieces).  Pinned
// text (pire_hip_host_alloc) is plain DMA at 57 GB/s.
constexpr size_t kHostChunkBytes = size_t(256) << 20;
constexpr size_t kHostChunkSlack = 4096;        // the kernels read whole 16-byte blocks around a string's ends
constexpr uint64_t kHostChunkStrings = 1u << 22;

struct HostArena {
	int device = -1;
	hipStream_t stream[2] = {nullptr, nullptr};
	hipEvent_t done[2] = {nullptr, nullptr};
	hipEvent_t ready = nullptr;
	// per slot, grown on demand
	uint8_t* text[2] = {nullptr, nullptr};
	size_t textCap[2] = {0, 0};
	uint64_t* offs[2] = {nullptr, nullptr};
	uint32_t* init[2] = {nullptr, nullptr};
	uint32_t* idx[2] = {nullptr, nullptr};
	uint8_t* fin[2] = {nullptr, nullptr};
	// results land in pinned host memory first: a device-to-host copy into the caller's (pageable) arrays would block
	// the host until the chunk's scan is over, and with it the transfer of the next chunk
	uint32_t* hostIdx[2] = {nullptr, nullptr};
	uint8_t* hostFin[2] = {nullptr, nullptr};
	size_t stringCap[2] = {0, 0};
	unsigned long long* counts = nullptr;
	size_t countBytes = 0;
};

std::mutex g_arenaMutex;
std::vector<HostArena*> g_arenas[kMaxDevices];

void FreeSlotStrings(HostArena* a, int k)
{
	(void)hipFree(a->offs[k]);
	(void)hipFree(a->init[k]);
	(void)hipFree(a->idx[k]);
	(void)hipFree(a->fin[k]);
	(void)hipHostFree(a->hostIdx[k]);
	(void)hipHostFree(a->hostFin[k]);
	a->offs[k] = nullptr;
	a->init[k] = a->idx[k] = a->hostIdx[k] = nullptr;
	a->fin[k] = a->hostFin[k] = nullptr;
	a->stringCap[k] = 0;
}

void DestroyArena(HostArena* a)
{
	for (int k = 0; k < 2; ++k) {
		if (a->stream[k])
			(void)hipStreamDestroy(a->stream[k]);
		if (a->done[k])
			(void)hipEventDestroy(a->done[k]);
		(void)hipFree(a->text[k]);
		FreeSlotStrings(a, k);
	}
	(void)hipFree(a->counts);
	if (a->ready)
		(void)hipEventDestroy(a->ready);
	delete a;
}

// Slot k of the arena can take `textBytes` of text and `strings` strings (the slot is idle when this is called).
int ReserveSlot(HostArena* a, int k, size_t textBytes, size_t strings)
{
	hipError_t e = hipSuccess;
	if (textBytes > a->textCap[k]) {
		(void)hipFree(a->text[k]);
		a->text[k] = nullptr;
		a->textCap[k] = 0;
		e = hipMalloc(reinterpret_cast<void**>(&a->text[k]), textBytes);
		if (e == hipSuccess)
			a->textCap[k] = textBytes;
	}
	if (e == hipSuccess && strings > a->stringCap[k]) {
		FreeSlotStrings(a, k);
		e = hipMalloc(reinterpret_cast<void**>(&a->offs[k]), (strings + 1) * 8);
		if (e == hipSuccess)
			e = hipMalloc(reinterpret_cast<void**>(&a->init[k]), strings * 4);
		if (e == hipSuccess)
			e = hipMalloc(reinterpret_cast<void**>(&a->idx[k]), strings * 4);
		if (e == hipSuccess)
			e = hipMalloc(reinterpret_cast<void**>(&a->fin[k]), strings);
		if (e == hipSuccess)
			e = hipHostMalloc(reinterpret_cast<void**>(&a->hostIdx[k]), strings * 4, hipHostMallocDefault);
		if (e == hipSuccess)
			e = hipHostMalloc(reinterpret_cast<void**>(&a->hostFin[k]), strings, hipHostMallocDefault);
		if (e == hipSuccess)
			a->stringCap[k] = strings;
	}
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "staging arena");
}

int AcquireArena(size_t countBytes, HostArena** out)
{
	int dev = -1;
	hipError_t e = hipGetDevice(&dev);
	if (e != hipSuccess || dev < 0 || dev >= kMaxDevices)
		return HipFail(e == hipSuccess ? hipErrorInvalidDevice : e, "hipGetDevice");
	{
		std::lock_guard<std::mutex> lock(g_arenaMutex);
		auto& pool = g_arenas[dev];
		for (size_t i = 0; i < pool.size(); ++i)
			if (pool[i]->countBytes >= countBytes) {
				*out = pool[i];
				pool.erase(pool.begin() + i);
				return PIRE_HIP_OK;
			}
	}
	std::unique_ptr<HostArena, void (*)(HostArena*)> a(new HostArena, DestroyArena);
	a->device = dev;
	a->countBytes = std::max<size_t>(countBytes, 1024);
	for (int k = 0; k < 2 && e == hipSuccess; ++k) {
		e = hipStreamCreateWithFlags(&a->stream[k], hipStreamNonBlocking);
		if (e == hipSuccess)
			e = hipEventCreateWithFlags(&a->done[k], hipEventDisableTiming);
	}
	if (e == hipSuccess)
		e = hipMalloc(reinterpret_cast<void**>(&a->counts), a->countBytes);
	if (e == hipSuccess)
		e = hipEventCreateWithFlags(&a->ready, hipEventDisableTiming);
	if (e != hipSuccess)
		return HipFail(e, "staging arena");
	*out = a.release();
	return PIRE_HIP_OK;
}

void ReleaseArena(HostArena* a)
{
	std::lock_guard<std::mutex> lock(g_arenaMutex);
	g_arenas[a->device].push_back(a);
}

// Returns PIRE_HIP_OK and *done = true when it handled the batch; *done = false (nothing touched) when the batch does
// not fit the chunking (a string longer than a chunk) and the caller should take the one-shot path.
int RunHostPipelined(pire_hip_table* t, const ScanParams& base, const uint8_t* text, const uint64_t* offsets, uint64_t n,
                     uint64_t len, uint64_t stride, const uint32_t* init, uint32_t* outIdx, uint8_t* outFinal,
                     uint64_t* outCounts, bool* done)
{
	*done = false;
	size_t chunkBytes = kHostChunkBytes;
	if (const uint64_t knob = GetConfig().host_chunk_bytes)   // tests: many small chunks
		chunkBytes = std::max<size_t>(4096, std::min<size_t>(kHostChunkBytes, size_t(knob)));
	// chunk boundaries: [first[c], first[c+1]) strings, text bytes [lo, hi) of the caller's buffer
	std::vector<uint64_t> first{0};
	if (offsets) {
		while (first.back() < n) {
			const uint64_t f = first.back();
			const uint64_t limit = offsets[f] + chunkBytes;
			uint64_t l = uint64_t(std::upper_bound(offsets + f + 1, offsets + n + 1, limit) - offsets) - 1;   // last string that still fits
			l = std::min<uint64_t>(l, f + kHostChunkStrings);
			if (l == f)
				return PIRE_HIP_OK;   // a single string larger than a chunk: not this path
			first.push_back(l);
		}
	} else {
		if (stride > chunkBytes / 64)
			return PIRE_HIP_OK;
		// stride 0 = n empty records (len == 0, pire_ut.cpp:832-837 semantics per record): chunk by string count alone
		uint64_t per = std::min<uint64_t>(stride ? chunkBytes / stride : kHostChunkStrings, kHostChunkStrings) & ~uint64_t(1023);
		if (per == 0)
			per = stride ? chunkBytes / stride : kHostChunkStrings;
		for (uint64_t f = per; f < n; f += per)
			first.push_back(f);
		first.push_back(n);
	}
	const size_t cntBytes = (size_t(t->host.regexps) + 2) * 8;
	HostArena* arena = nullptr;
	if (int rc = AcquireArena(cntBytes, &arena))
		return rc;
	struct Return {
		HostArena* a;
		~Return()
		{
			// whatever happened, nothing of this call may still be in flight when the arena goes back to the pool
			(void)hipStreamSynchronize(a->stream[0]);
			(void)hipStreamSynchronize(a->stream[1]);
			ReleaseArena(a);
		}
	} giveBack{arena};
	*done = true;
	hipError_t e = hipSuccess;
	if (outCounts) {
		// the counters are accumulated into: start from the caller's values, both streams wait for them
		e = hipMemcpyAsync(arena->counts, outCounts, cntBytes, hipMemcpyHostToDevice, arena->stream[0]);
		if (e == hipSuccess)
			e = hipEventRecord(arena->ready, arena->stream[0]);
		if (e == hipSuccess)
			e = hipStreamWaitEvent(arena->stream[1], arena->ready, 0);
		if (e != hipSuccess)
			return HipFail(e, "hipMemcpy(counts)");
	}
	// results of the chunk that used slot k last: out of the pinned staging into the caller's arrays
	auto drain = [&](size_t c) -> hipError_t {
		const int k = int(c & 1);
		hipError_t err = hipEventSynchronize(arena->done[k]);
		if (err != hipSuccess)
			return err;
		const uint64_t f = first[c], cnt = first[c + 1] - f;
		if (outIdx)
			memcpy(outIdx + f, arena->hostIdx[k], cnt * 4);
		if (outFinal)
			memcpy(outFinal + f, arena->hostFin[k], cnt);
		return hipSuccess;
	};
	const size_t chunks = first.size() - 1;
	for (size_t c = 0; c < chunks; ++c) {
		const int k = int(c & 1);
		hipStream_t s = arena->stream[k];
		const uint64_t f = first[c], cnt = first[c + 1] - f;
		if (c >= 2 && (e = drain(c - 2)) != hipSuccess)
			return HipFail(e, "hipEventSynchronize");
		{
			const uint64_t bytes = offsets ? offsets[f + cnt] - (offsets[f] & ~uint64_t(255)) : (cnt - 1) * stride + len;
			if (int rc = ReserveSlot(arena, k, size_t(bytes) + 2 * kHostChunkSlack, size_t(cnt)))
				return rc;
		}
		ScanParams p = base;
		p.n = cnt;
		uint64_t lo, hi;
		if (offsets) {
			lo = offsets[f] & ~uint64_t(255);   // keeps every string's alignment as it is in the caller's buffer
			hi = offsets[f + cnt];
			p.text = arena->text[k] - lo;       // so that the caller's offsets address the staged copy
			e = hipMemcpyAsync(arena->offs[k], offsets + f, (cnt + 1) * 8, hipMemcpyHostToDevice, s);
			p.offsets = arena->offs[k];
		} else {
			lo = f * stride;
			hi = (f + cnt - 1) * stride + len;
			p.text = arena->text[k];
			p.offsets = nullptr;
		}
		if (e == hipSuccess && hi > lo)
			e = hipMemcpyAsync(arena->text[k], text + lo, hi - lo, hipMemcpyHostToDevice, s);
		if (e == hipSuccess && init) {
			e = hipMemcpyAsync(arena->init[k], init + f, cnt * 4, hipMemcpyHostToDevice, s);
			p.initIdx = arena->init[k];
		}
		if (e != hipSuccess)
			return HipFail(e, "hipMemcpy(H2D)");
		p.outIdx = outIdx ? arena->idx[k] : nullptr;
		p.outFinal = outFinal ? arena->fin[k] : nullptr;
		p.outCounts = outCounts ? arena->counts : nullptr;
		if (int rc = Dispatch(p, s, NextWorkSlot(t, p), hi - lo))
			return rc;
		if (outIdx)
			e = hipMemcpyAsync(arena->hostIdx[k], arena->idx[k], cnt * 4, hipMemcpyDeviceToHost, s);
		if (e == hipSuccess && outFinal)
			e = hipMemcpyAsync(arena->hostFin[k], arena->fin[k], cnt, hipMemcpyDeviceToHost, s);
		if (e == hipSuccess)
			e = hipEventRecord(arena->done[k], s);
		if (e != hipSuccess)
			return HipFail(e, "hipMemcpy(D2H)");
	}
	for (size_t c = chunks >= 2 ? chunks - 2 : 0; c < chunks && e == hipSuccess; ++c)
		e = drain(c);
	if (e == hipSuccess && outCounts)
		e = hipMemcpy(outCounts, arena->counts, cntBytes, hipMemcpyDeviceToHost);
	if (e != hipSuccess)
		return HipFail(e, "copy back / synchronize");
	return PIRE_HIP_OK;
}

// Shared body of pire_hip_run / pire_hip_run_strided.
int RunImpl(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint64_t len, uint64_t stride,
            uint32_t flags, const uint32_t* init, uint32_t* outIdx, uint8_t* outFinal, uint64_t* outCounts,
            void* streamPtr)
{
	if (!t) {
		SetError("null table");
		return PIRE_HIP_EINVAL;
	}
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	// only the public bits: the upper ones are the kernels' internal switches (device_common.h)
	flags &= PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END | PIRE_HIP_RUN_ON_DEVICE | PIRE_HIP_RUN_GENERIC | PIRE_HIP_RUN_HOST_OFFSETS |
	         PIRE_HIP_RUN_NO_PEEK;
	ScanParams p;
	// (an automatic adaptation drains the device: only in calls that synchronise anyway, pire_hip_config.auto_adapt)
	TableUse use(t, (flags & PIRE_HIP_RUN_ON_DEVICE) && !(flags & PIRE_HIP_RUN_HOST_OFFSETS));
	if (int rc = FillParams(t, &p, flags))
		return rc;
	p.n = n;
	p.len = len;
	p.stride = stride;

	if (flags & PIRE_HIP_RUN_ON_DEVICE) {
		p.text = static_cast<const uint8_t*>(text);
		p.offsets = offsets;
		p.initIdx = init;
		p.outIdx = outIdx;
		p.outFinal = outFinal;
		p.outCounts = reinterpret_cast<unsigned long long*>(outCounts);
		if ((flags & PIRE_HIP_RUN_HOST_OFFSETS) && offsets && n) {
			// resident text, offsets known to the host
			return WithOffsetsOnDevice(offsets, n, stream, [&](const uint64_t* dOffsets) {
				p.offsets = dOffsets;
				const uint64_t textBytes = offsets[n];
				if (!(flags & PIRE_HIP_RUN_GENERIC) && SegmentedEligible(n, textBytes - offsets[0]))
					return RunSegmented(t, p, offsets, stream);
				return Dispatch(p, stream, NextWorkSlot(t, p), textBytes);
			});
		}
		// device offsets: the total text size is not known on the host; n >= 256 strings of unknown length still
		// need 128 readable bytes at `text` for the ragged kernel, which the caller guarantees by passing a batch
		// (a batch with less than 4 KiB of text is not worth a GPU launch; use PIRE_HIP_RUN_GENERIC to force the
		// offset-exact kernel)
		// Few long strings starve a one-string-per-lane kernel: cut them into segments (segmented.hip).  With
		// device offsets the host does not know the lengths, so only fixed-length records qualify here.
		if (!offsets && !(flags & PIRE_HIP_RUN_GENERIC) && n && SegmentedEligible(n, n * len))
			return RunSegmented(t, p, nullptr, stream);
		// Offsets on the device: the host does not know the lengths, and a handful of long strings would walk one per
		// lane at 25 MB/s each (a single 1 GiB string: 45 s against 0.5 ms segmented).  A batch small enough to leave
		// lanes idle (n < 65 536) is therefore PEEKED at: two words (first and last offset) come back -- which
		// synchronises `stream` -- and only if the cost model then asks for the segmented scan are all n + 1 offsets
		// fetched (<= 512 KB).  pire_hip_config.no_offsets_peek keeps such calls enqueue-only.
		if (offsets && n && n < 65536 && !(flags & (PIRE_HIP_RUN_GENERIC | PIRE_HIP_RUN_NO_PEEK)) && !GetConfig().no_offsets_peek) {
			uint64_t ends[2] = {0, 0};
			hipError_t e = hipMemcpyAsync(&ends[0], offsets, 8, hipMemcpyDeviceToHost, stream);
			if (e == hipSuccess)
				e = hipMemcpyAsync(&ends[1], offsets + n, 8, hipMemcpyDeviceToHost, stream);
			if (e == hipSuccess)
				e = hipStreamSynchronize(stream);
			if (e != hipSuccess)
				return HipFail(e, "reading the first and last offset back");
			const uint64_t total = ends[1] >= ends[0] ? ends[1] - ends[0] : 0;
			if (SegmentedEligible(n, total)) {
				std::vector<uint64_t> hostOffsets(size_t(n) + 1);
				e = hipMemcpyAsync(hostOffsets.data(), offsets, (size_t(n) + 1) * 8, hipMemcpyDeviceToHost, stream);
				if (e == hipSuccess)
					e = hipStreamSynchronize(stream);
				if (e != hipSuccess)
					return HipFail(e, "reading the offsets back");
				if (int rc = CheckOffsets(hostOffsets.data(), n))
					return rc;
				return RunSegmented(t, p, hostOffsets.data(), stream);
			}
			return Dispatch(p, stream, NextWorkSlot(t, p), total);
		}
		return Dispatch(p, stream, NextWorkSlot(t, p), offsets ? ~0ull : 0);
	}

	// Host-pointer mode (PCIe-inclusive; the benchmark never times this mode): through the chunked, pooled staging of
	// RunHostPipelined; few long strings (segmented scan), timed calls and strings larger than a chunk are staged in one
	// piece.
	if (n == 0)
		return PIRE_HIP_OK;
	Staging st(stream);
	uint64_t textBytes;
	if (int rc = CheckHostBatch(text, offsets, n, len, stride, &textBytes))
		return rc;
	if (init)
		for (uint64_t i = 0; i < n; ++i)
			if (init[i] >= t->host.states) {
				// host-side array: checking it costs nothing next to the transfer (device-side arrays are the caller's
				// responsibility, as a state is in the reference: Runner(sc, st) trusts st, run.h:368)
				SetError("init_state_idx out of range");
				return PIRE_HIP_EINVAL;
			}
	const bool segmented = !(flags & PIRE_HIP_RUN_GENERIC) && SegmentedEligible(n, textBytes);
	const size_t cntBytes = (size_t(t->host.regexps) + 2) * 8;
	// The pooled, chunked staging wins from a few hundred KiB on (3 MB 563 -> 308 us per call); a call whose inputs and
	// results all fit the one-piece staging's arena (internal.h, Staging: one copy in, one copy out) is faster there
	// (round 3: 10 strings 36 -> 30 us)
	const bool small = st.mode == 0 && textBytes + (n + 1) * 8 + n * 9 + cntBytes + 8 * 256 <= Staging::kArenaBytes;
	if (!segmented && !small && !g_timing && !GetConfig().host_one_shot) {
		bool done = false;
		const int rc = RunHostPipelined(t, p, static_cast<const uint8_t*>(text), offsets, n, len, stride, init, outIdx,
		                                outFinal, outCounts, &done);
		if (rc || done)
			return rc;
	}
	const uint8_t* dText = nullptr;
	if (int rc = st.In(static_cast<const uint8_t*>(text), size_t(textBytes), &dText, stream))
		return rc;
	p.text = dText;
	if (offsets)
		if (int rc = st.In(offsets, size_t(n + 1), &p.offsets, stream))
			return rc;
	if (init)
		if (int rc = st.In(init, size_t(n), &p.initIdx, stream))
			return rc;
	void* dIdx = nullptr;
	void* dFin = nullptr;
	const unsigned long long* dCnt = nullptr;
	if (outCounts) {   // accumulated into: an input as well as a result
		if (int rc = st.In(reinterpret_cast<const unsigned long long*>(outCounts), cntBytes / 8, &dCnt, stream))
			return rc;
		p.outCounts = const_cast<unsigned long long*>(dCnt);
	}
	if (outIdx) {
		if (int rc = st.Alloc(&dIdx, size_t(n) * 4))
			return rc;
		p.outIdx = static_cast<uint32_t*>(dIdx);
	}
	if (outFinal) {
		if (int rc = st.Alloc(&dFin, size_t(n)))
			return rc;
		p.outFinal = static_cast<uint8_t*>(dFin);
	}
	if (int rc = st.Flush())
		return rc;
	if (segmented) {
		if (int rc = RunSegmented(t, p, offsets, stream))
			return rc;
	} else if (int rc = Dispatch(p, stream, NextWorkSlot(t, p), textBytes)) {
		return rc;
	}
	if (int rc = st.Out(outIdx, dIdx, size_t(n) * 4))
		return rc;
	if (int rc = st.Out(outFinal, dFin, size_t(n)))
		return rc;
	if (int rc = st.Out(outCounts, dCnt, cntBytes))
		return rc;
	return st.Finish();
}

}  // namespace
}  // namespace pirehip

using namespace pirehip;

const char* pire_hip_selftested_kernels(void)
{
	static thread_local std::string copy;
	copy = SelfTestedKernels();
	return copy.c_str();
}

extern "C" {

int pire_hip_config_get(pire_hip_config* out)
{
	if (!out || out->size < sizeof(uint32_t)) {
		SetError("pire_hip_config_get: out->size must hold the caller's sizeof(pire_hip_config)");
		return PIRE_HIP_EINVAL;
	}
	const pire_hip_config c = GetConfig();
	const uint32_t n = std::min<uint32_t>(out->size, uint32_t(sizeof(c)));
	memcpy(out, &c, n);
	out->size = n;
	return PIRE_HIP_OK;
}

int pire_hip_config_set(const pire_hip_config* in)
{
	if (!in || in->size < sizeof(uint32_t)) {
		SetError("pire_hip_config_set: in->size must hold the caller's sizeof(pire_hip_config)");
		return PIRE_HIP_EINVAL;
	}
	std::lock_guard<std::mutex> lock(g_cfgMutex);
	pire_hip_config& c = ConfigStorage();
	memcpy(&c, in, std::min<size_t>(in->size, sizeof(c)));
	c.size = sizeof(c);
	return PIRE_HIP_OK;
}



const char* pire_hip_last_error(void) { return g_error.c_str(); }
const char* pire_hip_last_kernel(void) { return g_lastKernel; }
const char* pire_hip_last_kernel_symbol(void) { return g_lastSymbol ? g_lastSymbol : g_lastKernel; }

int pire_hip_set_timing(int enabled)
try {
	g_timing = enabled != 0;
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

float pire_hip_last_kernel_ms(void) { return g_lastMs; }

int pire_hip_device_count(void)
try {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) {
		(void)hipGetLastError();
		return 0;
	}
	return n;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_create(const void* save_blob, size_t len, pire_hip_table** out)
try {
	if (!out) {
		SetError("null out pointer");
		return PIRE_HIP_EINVAL;
	}
	*out = nullptr;
	std::unique_ptr<pire_hip_table> t(new (std::nothrow) pire_hip_table);
	if (!t) {
		SetError("out of memory");
		return PIRE_HIP_ENOMEM;
	}
	if (int rc = BuildHostTable(save_blob, len, &t->host))
		return rc;
	*out = t.release();
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_mmap(const void* image, size_t size, pire_hip_table** out, size_t* consumed)
try {
	if (consumed)
		*consumed = 0;
	const int rc = pire_hip_table_create(image, size, out);
	if (rc == PIRE_HIP_OK && consumed)
		*consumed = size_t((*out)->host.blobBytes);
	return rc;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_create_from_file(const char* path, pire_hip_table** out)
try {
	if (!path || !out) {
		SetError("null argument");
		return PIRE_HIP_EINVAL;
	}
	*out = nullptr;
	const int fd = open(path, O_RDONLY);
	if (fd < 0) {
		SetError(std::string("cannot open ") + path + ": " + strerror(errno));
		return PIRE_HIP_EINVAL;
	}
	struct stat st;
	if (fstat(fd, &st) != 0 || st.st_size <= 0) {
		SetError(std::string("cannot stat (or empty file) ") + path);
		close(fd);
		return PIRE_HIP_EFORMAT;
	}
	void* map = mmap(nullptr, size_t(st.st_size), PROT_READ, MAP_PRIVATE, fd, 0);
	close(fd);
	if (map == MAP_FAILED) {
		SetError(std::string("cannot mmap ") + path + ": " + strerror(errno));
		return PIRE_HIP_ENOMEM;
	}
	const int rc = pire_hip_table_create(map, size_t(st.st_size), out);   // the image is decoded, nothing aliases it
	munmap(map, size_t(st.st_size));
	return rc;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

namespace {

int GlueImpl(const pire_hip_table* lhs, const pire_hip_table* rhs, size_t max_size, pire_hip_table** out, bool onDevice)
{
	if (!lhs || !rhs || !out) {
		SetError("null argument");
		return PIRE_HIP_EINVAL;
	}
	*out = nullptr;
	std::unique_ptr<pire_hip_table> t(new (std::nothrow) pire_hip_table);
	if (!t) {
		SetError("out of memory");
		return PIRE_HIP_ENOMEM;
	}
	if (int rc = GlueHostTables(lhs->host, rhs->host, max_size, &t->host, onDevice))
		return rc;
	*out = t.release();
	return PIRE_HIP_OK;
}

}  // namespace

int pire_hip_table_glue_gpu(const pire_hip_table* lhs, const pire_hip_table* rhs, size_t max_size, pire_hip_table** out)
try {
	return GlueImpl(lhs, rhs, max_size, out, true);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_glue(const pire_hip_table* lhs, const pire_hip_table* rhs, size_t max_size, pire_hip_table** out)
try {
	return GlueImpl(lhs, rhs, max_size, out, false);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}


int pire_hip_table_upload(pire_hip_table* t)
try {
	if (!t) {
		SetError("null table");
		return PIRE_HIP_EINVAL;
	}
	std::shared_lock<std::shared_mutex> stable(t->adaptMutex);   // (an adaptation replaces t->host and the images)
	TableConfigScope scope;   // the image is built under the table's configuration, as an entry point would build it
	scope.Push(t);
	DeviceTable image;
	if (int rc = UploadTable(t, &image))
		return rc;
	// ... and what the counting walk of the same table (pire_hip_run_half_final) keeps on the device, when the table
	// qualifies for its row kernel: an ON_DEVICE call after this uploads nothing
	if (!t->host.empty && t->host.regexps && t->host.regexps <= 8)
		if (int rc = UploadHalfRows(t))
			return rc;
	// ... and the mask image of pire_hip_select (reference numbering: uploaded once per device, select.hip)
	return UploadSelect(t, nullptr);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_config_set(pire_hip_table* t, const pire_hip_config* in)
try {
	if (!t || (in && in->size < sizeof(uint32_t))) {
		SetError("pire_hip_table_config_set: null table, or in->size does not hold the caller's sizeof(pire_hip_config)");
		return PIRE_HIP_EINVAL;
	}
	const pire_hip_config now = GetConfig();
	std::unique_lock<std::shared_mutex> exclusive(t->adaptMutex);   // no entry point is looking at it
	if (!in) {
		t->hasConfig = false;
		return PIRE_HIP_OK;
	}
	t->config = now;   // fields beyond in->size: the process-wide values of this moment
	memcpy(&t->config, in, std::min<size_t>(in->size, sizeof(t->config)));
	t->config.size = sizeof(t->config);
	t->hasConfig = true;
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();
}

int pire_hip_table_config_get(const pire_hip_table* t, pire_hip_config* out)
try {
	if (!t || !out || out->size < sizeof(uint32_t)) {
		SetError("pire_hip_table_config_get: null argument, or out->size does not hold the caller's sizeof(pire_hip_config)");
		return PIRE_HIP_EINVAL;
	}
	pire_hip_config c = GetConfig();
	{
		std::shared_lock<std::shared_mutex> stable(const_cast<pire_hip_table*>(t)->adaptMutex);
		if (t->hasConfig)
			c = t->config;
	}
	const uint32_t n = std::min<uint32_t>(out->size, uint32_t(sizeof(c)));
	memcpy(out, &c, n);
	out->size = n;
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();
}

int pire_hip_table_adapt(pire_hip_table* t, uint32_t* changed_rows)
try {
	if (!t) {
		SetError("null table");
		return PIRE_HIP_EINVAL;
	}
	return AdaptTable(t, changed_rows);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_check_failures(pire_hip_table* t, uint64_t* out)
try {
	if (!t || !out) {
		SetError("null argument");
		return PIRE_HIP_EINVAL;
	}
	return CheckFailures(t, out);
} catch (...) {
	return pirehip::HandleException();
}

void pire_hip_table_destroy(pire_hip_table* t)
{
	if (!t)
		return;
	JoinBackgroundAdapt(t);
	FreeAllDeviceTables(t);
	FreeHalfRows(t);
	FreeSelect(t);
	if (t->segProduct)
		FreeAllDeviceTables(t->segProduct.get());   // the product automaton of the segmented scan's two modes
	delete t;
}

uint32_t pire_hip_abi_version(void) { return PIRE_HIP_ABI_VERSION; }

int pire_hip_table_get_info_sized(const pire_hip_table* t, void* out, size_t size)
try {
	if (!t || !out) {
		SetError("null argument");
		return PIRE_HIP_EINVAL;
	}
	pire_hip_table_info full;
	if (int rc = pire_hip_table_get_info(t, &full))
		return rc;
	memcpy(out, &full, std::min(size, sizeof(full)));
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();
}

int pire_hip_table_get_info(const pire_hip_table* t, pire_hip_table_info* out)
try {
	if (!t || !out) {
		SetError("null argument");
		return PIRE_HIP_EINVAL;
	}
	std::shared_lock<std::shared_mutex> stable(const_cast<pire_hip_table*>(t)->adaptMutex);
	EnsureRanked(const_cast<pire_hip_table*>(t));   // hot_states / lds_table_bytes describe the ranked device layout
	const HostTable& h = t->host;
	memset(out, 0, sizeof(*out));
	out->abi_version = PIRE_HIP_ABI_VERSION;
	out->states = h.states;
	out->letters = h.letters;
	out->regexps = h.regexps;
	out->initial = h.initial;
	out->empty = h.empty ? 1 : 0;
	out->header_size = h.headerSize;
	out->row_stride = h.rowStride;
	out->hot_states = h.hot;
	out->lds_table_bytes = MakeLayout(h.hot, 0, 256u, h.compact ? (h.compact + 1) * CompactPitch(h.letters) : 0).total;
	out->compact_states = h.compact;
	out->scanner_type = h.scannerType;
	out->zip_full_states = h.zipFull;
	out->zip_outside_share = h.zipOutside;
	out->zip_plain_outside_share = h.zipPlainOutside;
	out->wide_states = h.wide;
	out->wide_lds_bytes = h.wide ? MakeWideLayout(h.wide, h.letters, 0, h.zipFull).total : 0;
	out->outside_dense_share = h.outsideDense;
	out->outside_wide_share = h.outsideWide;
	out->shares_measured = h.massMeasured ? 1 : 0;
	out->last_wide_trap_chunks = h.lastWideTrapChunks;
	out->wide_outside_chunk_share = h.wideTwiceShare;
	out->device_bytes = 0;   // all images (one per device the table has run on)
	{
		// devs[] is written by the first run on a device, under uploadMutex (found by ThreadSanitizer, round 4: this loop
		// read it under the adaptation lock alone)
		std::lock_guard<std::mutex> images(const_cast<pire_hip_table*>(t)->uploadMutex);
		for (int k = 0; k < kMaxDevices; ++k)
			out->device_bytes += t->devs[k].device >= 0 ? t->devs[k].bytes : 0;
	}
	out->adaptations = h.adaptations;
	out->last_trap_samples = h.lastTrapSamples;
	out->ref_buf_size = h.refBufSize;
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// The accessors read t->host under adaptMutex SHARED: a swap in of a table ranked in the background replaces it (table.cpp
// BackgroundAdaptStep).  (Never from inside an entry point, which holds the lock already.)
static std::shared_lock<std::shared_mutex> HostLock(const pire_hip_table* t)
{
	return t ? std::shared_lock<std::shared_mutex>(const_cast<pire_hip_table*>(t)->adaptMutex) : std::shared_lock<std::shared_mutex>();
}

static int CheckIdx(const pire_hip_table* t, uint32_t idx)
{
	if (!t) {
		SetError("null table");
		return PIRE_HIP_EINVAL;
	}
	if (idx >= t->host.states) {
		SetError("state index out of range");
		return PIRE_HIP_EINVAL;
	}
	return PIRE_HIP_OK;
}

int pire_hip_table_final(const pire_hip_table* t, uint32_t idx)
try {
	const auto stable = HostLock(t);
	if (int rc = CheckIdx(t, idx))
		return rc;
	return (t->host.flags[idx] & kFinal) ? 1 : 0;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_dead(const pire_hip_table* t, uint32_t idx)
try {
	const auto stable = HostLock(t);
	if (int rc = CheckIdx(t, idx))
		return rc;
	return (t->host.flags[idx] & kDead) ? 1 : 0;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_accepted_regexps(const pire_hip_table* t, uint32_t idx, const uint64_t** begin, size_t* count)
try {
	const auto stable = HostLock(t);
	if (int rc = CheckIdx(t, idx))
		return rc;
	if (!begin || !count) {
		SetError("null argument");
		return PIRE_HIP_EINVAL;
	}
	const HostTable& h = t->host;
	*begin = h.acceptIds.data() + h.acceptOff[idx];
	*count = size_t(h.acceptOff[idx + 1] - h.acceptOff[idx]);
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_letter_class(const pire_hip_table* t, uint32_t ch)
try {
	if (!t || ch >= kMaxChar) {
		SetError("bad argument");
		return PIRE_HIP_EINVAL;
	}
	const auto stable = HostLock(t);
	return t->host.cls[ch];
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int64_t pire_hip_table_next(const pire_hip_table* t, uint32_t idx, uint32_t ch)
try {
	const auto stable = HostLock(t);
	if (int rc = CheckIdx(t, idx))
		return rc;
	if (ch >= kMaxCharUnaligned || ch == kEpsilon) {
		SetError("character out of range");
		return PIRE_HIP_EINVAL;
	}
	const HostTable& h = t->host;
	return h.next[size_t(idx) * h.letters + h.cls[ch]];
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_layout(const pire_hip_table* t, uint32_t* orig_of_perm, uint8_t* hot_rows)
try {
	if (!t) {
		SetError("null table");
		return PIRE_HIP_EINVAL;
	}
	std::shared_lock<std::shared_mutex> stable(const_cast<pire_hip_table*>(t)->adaptMutex);
	EnsureRanked(const_cast<pire_hip_table*>(t));
	const HostTable& h = t->host;
	if (orig_of_perm)
		memcpy(orig_of_perm, h.origOfPerm.data(), h.origOfPerm.size() * sizeof(uint32_t));
	if (hot_rows)
		memcpy(hot_rows, h.hotRows.data(), h.hotRows.size());
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_wide_layout(const pire_hip_table* t, uint16_t* rows, size_t cap, uint32_t* wide_states, uint32_t* pitch,
                               uint32_t* rows_offset)
try {
	if (!t) {
		SetError("null table");
		return PIRE_HIP_EINVAL;
	}
	std::shared_lock<std::shared_mutex> stable(const_cast<pire_hip_table*>(t)->adaptMutex);
	EnsureRanked(const_cast<pire_hip_table*>(t));
	const HostTable& h = t->host;
	const uint32_t wide = h.zipFull ? 0 : h.wide;   // a zipped image: pire_hip_table_zip_layout
	const WideLayout wl = MakeWideLayout(wide, h.letters, 0);
	if (wide_states)
		*wide_states = wide;
	if (pitch)
		*pitch = wl.pitch;
	if (rows_offset)
		*rows_offset = wl.rowsOff;
	if (rows && wide) {
		const std::vector<uint16_t> img = BuildWideRows(h);
		const size_t want = size_t(wide + 1) * wl.pitch / 2;
		if (cap < want) {
			SetError("wide layout: buffer too small");
			return PIRE_HIP_EINVAL;
		}
		memcpy(rows, img.data(), want * sizeof(uint16_t));
	}
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_table_zip_layout(const pire_hip_table* t, uint16_t* image, size_t cap, uint32_t geometry[8])
try {
	if (!t || !geometry) {
		SetError("null table / geometry");
		return PIRE_HIP_EINVAL;
	}
	std::shared_lock<std::shared_mutex> stable(const_cast<pire_hip_table*>(t)->adaptMutex);
	EnsureRanked(const_cast<pire_hip_table*>(t));
	const HostTable& h = t->host;
	memset(geometry, 0, 8 * sizeof(uint32_t));
	if (!h.zipFull)
		return PIRE_HIP_OK;
	const WideLayout wl = MakeWideLayout(h.wide, h.letters, 0, h.zipFull);
	const uint32_t g[8] = {h.wide, h.zipFull, wl.pitch, wl.rowsOff, wl.hOff, wl.xOff, wl.imageEnd, kZipExceptions};
	memcpy(geometry, g, sizeof(g));
	if (image) {
		const std::vector<uint16_t> img = BuildWideRows(h);
		const size_t want = (wl.imageEnd - wl.rowsOff) / 2;
		if (cap < want) {
			SetError("zip layout: buffer too small");
			return PIRE_HIP_EINVAL;
		}
		memcpy(image, img.data(), want * sizeof(uint16_t));
	}
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_run(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                 const uint32_t* init_state_idx, uint32_t* out_state_idx, uint8_t* out_final, uint64_t* out_counts,
                 void* stream)
try {
	if (n && !offsets) {
		SetError("null offsets");
		return PIRE_HIP_EINVAL;
	}
	if (offsets && !(flags & PIRE_HIP_RUN_ON_DEVICE) && n) {
		// fixed-length, 16-byte-friendly batches handed over as offsets still get the tiled kernel
		const uint64_t len = offsets[1] - offsets[0];
		bool uniform = offsets[0] == 0 && len >= 128 && len % 16 == 0;
		for (uint64_t i = 1; uniform && i < n; ++i)
			uniform = offsets[i + 1] - offsets[i] == len;
		if (uniform)
			return RunImpl(t, text, nullptr, n, len, len, flags, init_state_idx, out_state_idx, out_final,
			               out_counts, stream);
	}
	return RunImpl(t, text, offsets, n, 0, 0, flags, init_state_idx, out_state_idx, out_final, out_counts, stream);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_run_strided(pire_hip_table* t, const void* text, uint64_t n, uint64_t len, uint64_t stride,
                         uint32_t flags, const uint32_t* init_state_idx, uint32_t* out_state_idx, uint8_t* out_final,
                         uint64_t* out_counts, void* stream)
try {
	if (stride < len) {
		SetError("stride smaller than len");
		return PIRE_HIP_EINVAL;
	}
	return RunImpl(t, text, nullptr, n, len, stride, flags, init_state_idx, out_state_idx, out_final, out_counts,
	               stream);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- from end states to matches (select.hip, route.hip) ------------------------------------------------------------------
namespace {

// What pire_hip_select refuses before any device is touched
int SelectArgsInvalid(const pire_hip_table* t, const uint32_t* stateIdx, bool needIdx, uint64_t n, const uint64_t* outHits,
                      const uint64_t* outHitMasks, uint64_t hitCap, const uint64_t* outHitCount)
{
	const char* what = !t                           ? "null table"
	                   : needIdx && n && !stateIdx  ? "null state_idx"
	                   : !outHitCount               ? "null out_hit_count"
	                   : hitCap && !outHits         ? "hit_cap > 0 with null out_hits"
	                   : outHitMasks && !outHits    ? "out_hit_masks without out_hits"
	                                                : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string("pire_hip_select: ") + what);
	return PIRE_HIP_EINVAL;
}

// The front of the select and the route pass: the table's sizes (a snapshot under the lock), the host form's look at its
// state indices, the mask image of the current device.  *idle: a host call of no strings -- or, for a pass with a row per
// regexp, a table of none -- leaves the device nothing to do: no image is uploaded, no device is touched.
struct SelectImage {
	uint32_t states, words, regexps;
	SelectDevice device;
};
int SelectImageFor(const char* who, pire_hip_table* t, const uint32_t* stateIdx, uint64_t n, bool onDevice, bool rowPerRegexp,
                   SelectImage* image, bool* idle)
{
	{
		const std::shared_lock<std::shared_mutex> stable(t->adaptMutex);
		image->states = t->host.states;
		image->regexps = t->host.regexps;
		image->words = SelectMaskWords(image->regexps);
	}
	if (!onDevice)
		for (uint64_t i = 0; i < n; ++i)
			if (stateIdx[i] >= image->states) {
				SetError(std::string(who) + ": state_idx out of range");
				return PIRE_HIP_EINVAL;
			}
	*idle = (!onDevice && n == 0) || (rowPerRegexp && image->regexps == 0);
	if (*idle)
		return PIRE_HIP_OK;
	// (the image is in reference numbering: built once, whatever re-rankings come; the lock is for reading t->host)
	const std::shared_lock<std::shared_mutex> stable(t->adaptMutex);
	return UploadSelect(t, &image->device);
}

// Host pointers: the lists of a pass come back only as far as they were written -- row r of dev[rows][staged] (entries of
// `width` bytes) into row r of out[rows][pitch], its first min(counts[r], staged) entries.  dev == nullptr: nothing.  (The
// row-pitch form of HitStage::Back, for the lists that a LinesFrame stages and the rows of a route.)
int HitsBack(uint32_t rows, const uint64_t* counts, uint64_t staged, uint64_t pitch, const void* dev, void* out, size_t width, const char* what)
{
	for (uint32_t r = 0; r < rows && dev; ++r)
		if (const uint64_t written = std::min(counts[r], staged)) {
			const hipError_t e = hipMemcpy(static_cast<uint8_t*>(out) + uint64_t(r) * pitch * width,
			                               static_cast<const uint8_t*>(dev) + uint64_t(r) * staged * width, size_t(written) * width, hipMemcpyDeviceToHost);
			if (e != hipSuccess)
				return HipFail(e, what);
		}
	return PIRE_HIP_OK;
}

int SelectImpl(pire_hip_table* t, const uint32_t* stateIdx, uint64_t n, const uint64_t* want, uint32_t flags,
               uint64_t* outMasks, uint64_t* outHits, uint64_t* outHitMasks, uint64_t hitCap, uint64_t* outHitCount,
               hipStream_t stream)
{
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	SelectImage image;
	bool idle;
	if (int rc = SelectImageFor("pire_hip_select", t, stateIdx, n, onDevice, false, &image, &idle))
		return rc;
	if (idle) {
		*outHitCount = 0;
		return PIRE_HIP_OK;
	}
	const uint32_t words = image.words;
	// host pointers: staged in, the three kernels, staged out -- the hits only as far as they were written
	BatchIO io(stream, onDevice);
	const uint32_t* dIdx = nullptr;
	const uint64_t* dWant = nullptr;
	if (int rc = io.In(stateIdx, size_t(n), &dIdx))
		return rc;
	if (want)
		if (int rc = io.In(want, size_t(words), &dWant))
			return rc;
	const uint64_t cap = std::min<uint64_t>(hitCap, n);   // n strings have at most n hits: a host call stages no more
	uint64_t *dCount = nullptr, *dMasks = nullptr, *dHits = nullptr, *dHitMasks = nullptr;
	if (int rc = io.Result(outHitCount, 1, 1, &dCount))   // (the count comes back first: it says how far the lists were written)
		return rc;
	if (outMasks)
		if (int rc = io.Result(outMasks, size_t(n) * words, size_t(n) * words, &dMasks))
			return rc;
	if (outHits && cap)
		if (int rc = io.Result(outHits, size_t(cap), 0, &dHits))
			return rc;
	if (outHitMasks && cap)
		if (int rc = io.Result(outHitMasks, size_t(cap) * words, 0, &dHitMasks))
			return rc;
	if (int rc = io.Ready())
		return rc;
	if (int rc = LaunchSelect(image.device, image.states, words, dIdx, n, dWant, dMasks, dHits, dHitMasks, dHits ? cap : 0, dCount, stream))
		return rc;
	if (int rc = io.Finish())
		return rc;
	if (onDevice)
		return PIRE_HIP_OK;
	if (int rc = HitsBack(1, outHitCount, cap, cap, dHits, outHits, 8, "hipMemcpy(hits)"))
		return rc;
	return HitsBack(1, outHitCount, cap, cap, dHits ? dHitMasks : nullptr, outHitMasks, size_t(words) * 8, "hipMemcpy(hits)");
}

// pire_hip_run[_strided] followed by a pass over its state indices on the same stream: the one owner of the state-index
// array where the caller has none -- a vector with host pointers, stream-ordered scratch on the device.  `run` makes the scan
// call with the array it is given, `pass` the select or the route call (its flags: ON_DEVICE or nothing).
// (Whatever staging path the scan takes -- chunked, one piece, segmented --, its state indices arrive in ONE host array
// before the pass sees them: hit indices are relative to the whole batch.)
int RunThenPass(uint64_t n, uint32_t flags, uint32_t* outIdx, hipStream_t stream, const std::function<int(uint32_t*)>& run,
                const std::function<int(const uint32_t*, uint32_t)>& pass)
{
	const uint32_t onDevice = flags & PIRE_HIP_RUN_ON_DEVICE;
	std::vector<uint32_t> own;
	StreamScratch scratch(stream);
	if (!outIdx && !onDevice) {
		own.resize(size_t(n));
		outIdx = own.data();
	} else if (!outIdx && n) {
		if (int rc = scratch.Alloc(size_t(n) * 4, "hipMallocAsync(state indices)"))
			return rc;
		outIdx = scratch.as<uint32_t>();
	}
	if (int rc = run(outIdx))
		return rc;
	return pass(outIdx, onDevice);
}

int RunSelectImpl(pire_hip_table* t, uint64_t n, const uint64_t* want, uint32_t flags, uint32_t* outIdx, uint64_t* outMasks,
                  uint64_t* outHits, uint64_t* outHitMasks, uint64_t hitCap, uint64_t* outHitCount, void* streamPtr,
                  const std::function<int(uint32_t*)>& run)
{
	if (int rc = SelectArgsInvalid(t, nullptr, false, n, outHits, outHitMasks, hitCap, outHitCount))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	return RunThenPass(n, flags, outIdx, stream, run, [&](const uint32_t* idx, uint32_t passFlags) {
		return SelectImpl(t, idx, n, want, passFlags, outMasks, outHits, outHitMasks, hitCap, outHitCount, stream);
	});
}

uint32_t HostRegexps(const pire_hip_table* t)
{
	const auto stable = HostLock(t);
	return t->host.regexps;
}

// What the route entry points refuse before any device is touched
int RouteArgsInvalid(const char* who, const pire_hip_table* t, const uint32_t* stateIdx, bool needIdx, uint64_t n,
                     const uint64_t* outHits, const uint64_t* outHitSpans, uint64_t hitCap, const uint64_t* outHitCounts)
{
	const char* what = !t                                             ? "null table"
	                   : needIdx && n && !stateIdx                    ? "null state_idx"
	                   : !outHitCounts && HostRegexps(t)              ? "null out_hit_counts"
	                   : hitCap && !outHits                           ? "hit_cap > 0 with null out_hits"
	                   : outHitSpans && !outHits                      ? "out_hit_spans without out_hits"
	                                                                  : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

int RouteImpl(pire_hip_table* t, const uint32_t* stateIdx, uint64_t n, uint32_t flags, uint64_t* outHits, uint64_t hitCap,
              uint64_t* outHitCounts, hipStream_t stream)
{
	if (n >= (1ull << 32)) {
		SetError("pire_hip_route: 2^32 strings or more in one call");
		return PIRE_HIP_EUNSUPPORTED;
	}
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	SelectImage image;
	bool idle;
	if (int rc = SelectImageFor("pire_hip_route", t, stateIdx, n, onDevice, true, &image, &idle))
		return rc;
	const uint32_t regexps = image.regexps;
	if (idle) {
		if (regexps)   // (no rows: nothing to write)
			std::fill(outHitCounts, outHitCounts + regexps, uint64_t(0));
		return PIRE_HIP_OK;
	}
	// host pointers: staged in, the three kernels, staged out -- the rows at a pitch of their own, min(hit_cap, n)
	BatchIO io(stream, onDevice);
	const uint32_t* dIdx = nullptr;
	if (int rc = io.In(stateIdx, size_t(n), &dIdx))
		return rc;
	const uint64_t cap = onDevice ? hitCap : std::min<uint64_t>(hitCap, n);
	uint64_t *dCounts = nullptr, *dHits = nullptr;
	if (int rc = io.Result(outHitCounts, regexps, regexps, &dCounts))
		return rc;
	if (outHits && cap)
		if (int rc = io.Result(outHits, size_t(regexps) * size_t(cap), 0, &dHits))
			return rc;
	if (int rc = io.Ready())
		return rc;
	if (int rc = LaunchRoute(image.device, image.states, image.words, regexps, dIdx, n, dHits, dHits ? cap : 0, dCounts, stream))
		return rc;
	if (int rc = io.Finish())
		return rc;
	// (the caller's pitch stays hitCap)
	return onDevice ? PIRE_HIP_OK : HitsBack(regexps, outHitCounts, cap, hitCap, dHits, outHits, 8, "hipMemcpy(route hits)");
}

int RunRouteImpl(const char* who, pire_hip_table* t, uint64_t n, uint32_t flags, uint32_t* outIdx, uint64_t* outHits, uint64_t hitCap,
                 uint64_t* outHitCounts, void* streamPtr, const std::function<int(uint32_t*)>& run)
{
	if (int rc = RouteArgsInvalid(who, t, nullptr, false, n, outHits, nullptr, hitCap, outHitCounts))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	return RunThenPass(n, flags, outIdx, stream, run, [&](const uint32_t* idx, uint32_t passFlags) {
		return RouteImpl(t, idx, n, passFlags, outHits, hitCap, outHitCounts, stream);
	});
}

}  // namespace

uint32_t pire_hip_table_mask_words(const pire_hip_table* t)
try {
	const auto stable = HostLock(t);
	return t ? SelectMaskWords(t->host.regexps) : 0;
} catch (...) {
	pirehip::HandleException();
	return 0;
}

int pire_hip_select(pire_hip_table* t, const uint32_t* state_idx, uint64_t n, const uint64_t* want, uint32_t flags,
                    uint64_t* out_masks, uint64_t* out_hits, uint64_t* out_hit_masks, uint64_t hit_cap,
                    uint64_t* out_hit_count, void* stream)
try {
	if (int rc = SelectArgsInvalid(t, state_idx, true, n, out_hits, out_hit_masks, hit_cap, out_hit_count))
		return rc;
	return SelectImpl(t, state_idx, n, want, flags, out_masks, out_hits, out_hit_masks, hit_cap, out_hit_count,
	                  static_cast<hipStream_t>(stream));
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_run_select(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                        const uint32_t* init_state_idx, uint32_t* out_state_idx, uint8_t* out_final, uint64_t* out_counts,
                        const uint64_t* want, uint64_t* out_masks, uint64_t* out_hits, uint64_t* out_hit_masks,
                        uint64_t hit_cap, uint64_t* out_hit_count, void* stream)
try {
	return RunSelectImpl(t, n, want, flags, out_state_idx, out_masks, out_hits, out_hit_masks, hit_cap, out_hit_count, stream,
	                     [&](uint32_t* idx) {
		                     return pire_hip_run(t, text, offsets, n, flags, init_state_idx, idx, out_final, out_counts, stream);
	                     });
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_run_select_strided(pire_hip_table* t, const void* text, uint64_t n, uint64_t len, uint64_t stride, uint32_t flags,
                                const uint32_t* init_state_idx, uint32_t* out_state_idx, uint8_t* out_final,
                                uint64_t* out_counts, const uint64_t* want, uint64_t* out_masks, uint64_t* out_hits,
                                uint64_t* out_hit_masks, uint64_t hit_cap, uint64_t* out_hit_count, void* stream)
try {
	return RunSelectImpl(t, n, want, flags, out_state_idx, out_masks, out_hits, out_hit_masks, hit_cap, out_hit_count, stream,
	                     [&](uint32_t* idx) {
		                     return pire_hip_run_strided(t, text, n, len, stride, flags, init_state_idx, idx, out_final, out_counts,
		                                                 stream);
	                     });
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_route(pire_hip_table* t, const uint32_t* state_idx, uint64_t n, uint32_t flags, uint64_t* out_hits, uint64_t hit_cap,
                   uint64_t* out_hit_counts, void* stream)
try {
	if (int rc = RouteArgsInvalid("pire_hip_route", t, state_idx, true, n, out_hits, nullptr, hit_cap, out_hit_counts))
		return rc;
	return RouteImpl(t, state_idx, n, flags, out_hits, hit_cap, out_hit_counts, static_cast<hipStream_t>(stream));
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_run_route(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                       const uint32_t* init_state_idx, uint32_t* out_state_idx, uint8_t* out_final, uint64_t* out_counts,
                       uint64_t* out_hits, uint64_t hit_cap, uint64_t* out_hit_counts, void* stream)
try {
	return RunRouteImpl("pire_hip_run_route", t, n, flags, out_state_idx, out_hits, hit_cap, out_hit_counts, stream, [&](uint32_t* idx) {
		return pire_hip_run(t, text, offsets, n, flags, init_state_idx, idx, out_final, out_counts, stream);
	});
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_run_route_strided(pire_hip_table* t, const void* text, uint64_t n, uint64_t len, uint64_t stride, uint32_t flags,
                               const uint32_t* init_state_idx, uint32_t* out_state_idx, uint8_t* out_final, uint64_t* out_counts,
                               uint64_t* out_hits, uint64_t hit_cap, uint64_t* out_hit_counts, void* stream)
try {
	return RunRouteImpl("pire_hip_run_route_strided", t, n, flags, out_state_idx, out_hits, hit_cap, out_hit_counts, stream,
	                    [&](uint32_t* idx) {
		                    return pire_hip_run_strided(t, text, n, len, stride, flags, init_state_idx, idx, out_final, out_counts,
		                                                stream);
	                    });
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- raw text into strings (split.hip) -----------------------------------------------------------------------------------
namespace {

// What both split entry points refuse before any device is touched (`count`: out_n / out_line_count)
int SplitArgsInvalid(const char* who, const void* raw, uint64_t size, uint32_t delim, const void* count, const char* countName)
{
	std::string what = delim > 255      ? "delim > 255"
	                   : !count         ? std::string("null ") + countName
	                   : size && !raw   ? "size > 0 with null raw"
	                                    : "";
	if (what.empty())
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

// The number of strings, from the device to the host in the middle of a call: the stream is drained
int ReadCount(const uint64_t* dev, uint64_t* host, hipStream_t stream)
{
	hipError_t e = hipMemcpyAsync(host, dev, 8, hipMemcpyDeviceToHost, stream);
	if (e == hipSuccess)
		e = hipStreamSynchronize(stream);
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "reading the number of strings back");
}

// What the passes that are not in-place refuse: outText[0, textCap) over source[0, size)
int GatherOverlaps(const char* who, const void* source, uint64_t size, const void* outText, uint64_t textCap,
                   const char* what = "out_text overlaps the source (the pass is not in-place)")
{
	const uintptr_t r = reinterpret_cast<uintptr_t>(source), o = reinterpret_cast<uintptr_t>(outText);
	if (!(outText && size && textCap && o < r + size && r < o + textCap))
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

}  // namespace

int pire_hip_split(const void* raw, uint64_t size, uint32_t delim, uint32_t flags, void* out_text, uint64_t* out_offsets,
                   uint64_t offsets_cap, uint64_t* out_n, void* streamPtr)
try {
	if (int rc = SplitArgsInvalid("pire_hip_split", raw, size, delim, out_n, "out_n"))
		return rc;
	if (offsets_cap && !out_offsets) {
		SetError("pire_hip_split: offsets_cap > 0 with null out_offsets");
		return PIRE_HIP_EINVAL;
	}
	if (int rc = GatherOverlaps("pire_hip_split", raw, size, out_text, size, "out_text overlaps raw (the pass is not in-place)"))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	if (!onDevice && size == 0) {
		*out_n = 0;
		if (out_offsets)
			out_offsets[0] = 0;
		return PIRE_HIP_OK;
	}
	BatchIO io(stream, onDevice);
	const uint8_t* dRaw = nullptr;
	if (int rc = io.In(static_cast<const uint8_t*>(raw), size_t(size), &dRaw))
		return rc;
	uint64_t n = 0;   // host pointers: the count comes back here first
	uint64_t* dN = nullptr;
	if (int rc = io.Result(onDevice ? out_n : &n, 1, 1, &dN))
		return rc;
	if (int rc = io.Ready())
		return rc;
	StreamScratch scratch(stream);
	SplitPlan plan;
	if (int rc = LaunchSplitCount(dRaw, size, delim, dN, stream, scratch, &plan))
		return rc;
	if (onDevice)
		return LaunchSplitScatter(plan, out_text, out_offsets, offsets_cap, dN, stream);
	// host pointers: n first -- it says how much there is to stage
	if (int rc = ReadCount(dN, &n, stream))
		return rc;
	const uint64_t delims = n - (static_cast<const uint8_t*>(raw)[size - 1] != delim ? 1 : 0);
	const uint64_t entries = std::min(n, offsets_cap);
	uint8_t* dText = nullptr;
	uint64_t* dOffsets = nullptr;
	if (out_text)
		if (int rc = io.Result(static_cast<uint8_t*>(out_text), size_t(size - delims), size_t(size - delims), &dText))
			return rc;
	if (out_offsets)
		if (int rc = io.Result(out_offsets, size_t(entries) + 1, size_t(entries) + 1, &dOffsets))
			return rc;
	if (int rc = LaunchSplitScatter(plan, dText, dOffsets, entries, dN, stream))
		return rc;
	if (int rc = io.Finish())
		return rc;
	*out_n = n;
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

namespace {

// What the gather forms of the lines entry points add: where the bytes of the selected lines go, and which lists the frame
// keeps in scratch of its own where the caller has no array for them (the spans always; the hits where the pass writes
// its spans from them)
struct LinesGather {
	uint32_t tail;
	void* outText;
	uint64_t textCap;
	uint64_t* outOffsets;
	uint64_t* outBytes;
	bool needHits;
	const char* spansLabel;
};

// What the gather entry points refuse of their outputs before any device is touched.  capAlias: what this entry point
// calls idx_cap where it has another name for it (the message names both), else nullptr.
int GatherOutputsInvalid(const char* who, const char* capAlias, uint64_t cap, uint32_t tail, const void* outText, uint64_t textCap,
                         const void* outOffsets, const void* outBytes)
{
	const char* what = !outBytes                                      ? "null out_bytes"
	                   : tail != PIRE_HIP_GATHER_NO_TAIL && tail > 255 ? "tail > 255"
	                   : cap && !outOffsets                            ? "idx_cap > 0 with null out_offsets"
	                   : textCap && !outText                           ? "text_cap > 0 with null out_text"
	                                                                   : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	const bool aliased = capAlias && cap && !outOffsets && outBytes && !(tail != PIRE_HIP_GATHER_NO_TAIL && tail > 255);
	SetError(std::string(who) + ": " + what + (aliased ? std::string(" (idx_cap = ") + capAlias + ")" : ""));
	return PIRE_HIP_EINVAL;
}

int GatherRefuse(const char* who, const char* what)
{
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

// The lines of a raw buffer as text + offsets in scratch of the library's own, for the scan of a lines form: the split's
// count and scan, n read back (*dN and *n: the one wait of such a call, it sizes the offsets), the split's scatter
struct LinesScratch {
	StreamScratch tiles, text, offsets;
	explicit LinesScratch(hipStream_t s) : tiles(s), text(s), offsets(s) {}
};
int SplitLines(const char* who, const uint8_t* dRaw, uint64_t size, uint32_t delim, uint64_t* dN, uint64_t* n, hipStream_t stream,
               LinesScratch& out)
{
	SplitPlan plan;
	if (int rc = LaunchSplitCount(dRaw, size, delim, dN, stream, out.tiles, &plan))
		return rc;
	if (int rc = ReadCount(dN, n, stream))
		return rc;
	if (*n >= (1ull << 32)) {
		SetError(std::string(who) + ": 2^32 lines or more in one call");
		return PIRE_HIP_EUNSUPPORTED;
	}
	if (int rc = out.text.Alloc(size_t(size) + 16, "hipMallocAsync(split text)"))
		return rc;
	if (int rc = out.offsets.Alloc((size_t(*n) + 1) * 8, "hipMallocAsync(split offsets)"))
		return rc;
	return LaunchSplitScatter(plan, out.text.get(), out.offsets.as<uint64_t>(), *n, dN, stream);
}

// The column a field form of the lines entry points scans instead of the whole line (pire_hip_fields' arguments)
struct LinesField {
	uint32_t sep, field, mode;
};

// What pire_hip_fields and the field forms refuse of the column before any device is touched
int FieldArgsInvalid(const char* who, uint32_t sep, uint32_t mode)
{
	const char* what = sep > 255 ? "sep > 255" : mode & ~PIRE_HIP_FIELDS_REST ? "unknown bits in mode" : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

// The frame of the lines entry points (pire_hip_run_lines_select / _gather and their field forms, pire_hip_run_lines_route,
// pire_hip_capture_lines_gather) around their scan + pass: raw bytes in, hit lists (and, in the gather forms, the bytes of the
// hits) out.  An entry point checks its arguments, then walks the frame's steps in this order:
//   HostEdge   an empty buffer with host pointers: the line count and the gather's outputs are zeroed, no device is touched
//   Open       raw staged in (inputs of the entry point's own go in behind it: the select form's `want`)
//   Split      the line count, `rows` hit counts and the byte count staged to come back first; SplitLines -- the call's one
//              wait --; cap: no list is longer than the lines are many
//   Lists      hits[rows][cap] and spans[rows][cap][2] staged at size 0 where the caller has arrays for them; a gather form:
//              scratch for the lists it chains on and the caller did not ask for, out_text and out_offsets
//   Cut        a field form, n > 0: pire_hip_fields on the lines and the gather of the n fields into scratch; Text() and
//              Offsets() are that batch from here on -- string k of it is the column of line k --, LineOffsets() stays the split's
//   -- the entry point enqueues its scan + pass on the lines (Text(), Offsets(), n, cap, RunFlags()) into dCounts / dHits / dSpans --
//   Close      a gather form: the gather straight from raw through the spans; Finish(); host pointers: the line count, and
//              the lists, offsets and text back only as far as they were written (HitsBack)
struct LinesFrame {
	const char* who;
	const uint8_t* raw;
	uint64_t size;
	uint32_t delim, flags;
	const LinesGather* gather;   // nullable
	hipStream_t stream;
	bool onDevice;
	BatchIO io;
	LinesScratch lines;
	StreamScratch ownHits, ownSpans, cut;
	const uint8_t* cutText = nullptr;      // the fields back to back, their offsets: what a field form scans
	const uint64_t* cutOffsets = nullptr;
	uint64_t n = 0, cap = 0, hitCap = 0, textRoom = 0;   // textRoom of out_text: k lines and their tails are size + k bytes at most
	uint32_t rows = 0;
	uint64_t *outLineCount = nullptr, *outCounts = nullptr, *outHits = nullptr, *outSpans = nullptr;
	const uint8_t* dRaw = nullptr;
	uint64_t *dN = nullptr, *dCounts = nullptr, *dHits = nullptr, *dSpans = nullptr, *dBytes = nullptr, *dOutOffsets = nullptr;
	uint8_t* dOutText = nullptr;

	LinesFrame(const char* who_, const void* raw_, uint64_t size_, uint32_t delim_, uint32_t flags_, const LinesGather* gather_, void* stream_)
		: who(who_), raw(static_cast<const uint8_t*>(raw_)), size(size_), delim(delim_), flags(flags_), gather(gather_),
		  stream(static_cast<hipStream_t>(stream_)), onDevice((flags_ & PIRE_HIP_RUN_ON_DEVICE) != 0), io(stream, onDevice), lines(stream),
		  ownHits(stream), ownSpans(stream), cut(stream)
	{
	}
	const void* Text() const { return cutText ? cutText : lines.text.get(); }
	const uint64_t* Offsets() const { return cutOffsets ? cutOffsets : LineOffsets(); }
	const uint64_t* LineOffsets() const { return lines.offsets.as<uint64_t>(); }
	uint32_t RunFlags() const { return (flags & (PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END | PIRE_HIP_RUN_GENERIC)) | PIRE_HIP_RUN_ON_DEVICE; }

	bool HostEdge(uint64_t* lineCount)
	{
		if (onDevice || size)
			return false;
		*lineCount = 0;
		if (gather) {
			*gather->outBytes = 0;
			if (gather->outOffsets)
				gather->outOffsets[0] = 0;
		}
		return true;
	}
	int Open() { return io.In(raw, size_t(size), &dRaw); }
	// capByLines: false where a device caller's pitch has to stay hit_cap itself (the route form's rows)
	int Split(uint64_t* lineCount, uint64_t* counts, uint32_t rows_, uint64_t hitCap_, bool capByLines)
	{
		outLineCount = lineCount, outCounts = counts, rows = rows_, hitCap = hitCap_;
		if (int rc = io.Result(onDevice ? lineCount : &n, 1, 1, &dN))   // (host pointers: n comes back here first)
			return rc;
		if (rows)
			if (int rc = io.Result(counts, rows, rows, &dCounts))
				return rc;
		if (gather)
			if (int rc = io.Result(gather->outBytes, 1, 1, &dBytes))
				return rc;
		if (int rc = io.Ready())
			return rc;
		// the split, into scratch that lives until the scan and the gather behind it are enqueued; n sizes the offsets
		if (int rc = SplitLines(who, dRaw, size, delim, dN, &n, stream, lines))
			return rc;
		cap = capByLines ? std::min<uint64_t>(hitCap, n) : hitCap;   // n lines have at most n hits
		return PIRE_HIP_OK;
	}
	int Lists(uint64_t* hits, uint64_t* spans)
	{
		outHits = hits, outSpans = spans;
		const size_t entries = size_t(rows) * size_t(cap);
		if (hits && entries)
			if (int rc = io.Result(hits, entries, 0, &dHits))
				return rc;
		if (spans && entries)
			if (int rc = io.Result(spans, entries * 2, 0, &dSpans))
				return rc;
		if (!gather)
			return PIRE_HIP_OK;
		if (cap) {
			if (!dHits && gather->needHits) {
				if (int rc = ownHits.Alloc(size_t(cap) * 8, "hipMallocAsync(hits)"))
					return rc;
				dHits = ownHits.as<uint64_t>();
			}
			if (!dSpans) {
				if (int rc = ownSpans.Alloc(size_t(cap) * 16, gather->spansLabel))
					return rc;
				dSpans = ownSpans.as<uint64_t>();
			}
			textRoom = std::min(gather->textCap, size + cap);
			if (textRoom)
				if (int rc = io.Result(static_cast<uint8_t*>(gather->outText), size_t(textRoom), 0, &dOutText))
					return rc;
		}
		return gather->outOffsets ? io.Result(gather->outOffsets, size_t(cap) + 1, 0, &dOutOffsets) : PIRE_HIP_OK;
	}
	int Cut(const LinesField& c) { return Cut(c, cut); }
	// (a form that scans several columns cuts once per column, each cut into an owner of its own that it keeps alive until its
	// scans are enqueued; Text() and Offsets() are the latest cut)
	int Cut(const LinesField& c, StreamScratch& owner)
	{
		// one block: spans[n][2], offsets[n + 1], the byte count, the text (no longer than the lines are)
		const size_t words = size_t(n) * 3 + 2;
		if (int rc = owner.Alloc(words * 8 + size_t(size) + 16, "hipMallocAsync(fields)"))
			return rc;
		uint64_t* spans = owner.as<uint64_t>();
		uint64_t* offsets = spans + 2 * n;
		uint64_t* bytes = offsets + n + 1;
		uint8_t* text = reinterpret_cast<uint8_t*>(bytes + 1);
		if (int rc = LaunchFields(lines.text.get(), LineOffsets(), n, c.sep, c.field, c.mode, spans, size, stream))
			return rc;
		const GatherSource src = {lines.text.as<const uint8_t>(), nullptr, 0, nullptr, spans, size};
		if (int rc = LaunchGather(src, nullptr, n, PIRE_HIP_GATHER_NO_TAIL, text, size, offsets, bytes, kGatherTotalUnknown, stream))
			return rc;
		cutText = text, cutOffsets = offsets;
		return PIRE_HIP_OK;
	}
	// n == 0: the hit counts are zeroed where the entry point has no pass to do it
	int ZeroCounts(const char* what)
	{
		const hipError_t e = rows ? hipMemsetAsync(dCounts, 0, size_t(rows) * 8, stream) : hipSuccess;
		return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, what);
	}
	int Close(const char* backLabel)
	{
		if (gather) {
			// straight from raw, through the spans (cap == 0: *out_bytes = 0 and out_offsets[0] = 0, nothing is read)
			const GatherSource src = {dRaw, nullptr, 0, nullptr, dSpans, size};
			if (int rc = LaunchGather(src, dCounts, cap, gather->tail, dOutText, textRoom, dOutOffsets, dBytes, kGatherTotalUnknown, stream))
				return rc;
		}
		if (int rc = io.Finish())
			return rc;
		if (onDevice)
			return PIRE_HIP_OK;
		*outLineCount = n;
		// (the caller's pitch stays hit_cap where the staged rows are cap long)
		if (int rc = HitsBack(rows, outCounts, cap, hitCap, outHits ? dHits : nullptr, outHits, 8, backLabel))
			return rc;
		if (int rc = HitsBack(rows, outCounts, cap, hitCap, outSpans ? dSpans : nullptr, outSpans, 16, backLabel))
			return rc;
		if (!gather)
			return PIRE_HIP_OK;
		const uint64_t written = std::min(outCounts[0], cap), bytes = std::min(*gather->outBytes, textRoom);
		hipError_t e = hipSuccess;
		if (dOutOffsets)
			e = hipMemcpy(gather->outOffsets, dOutOffsets, (size_t(written) + 1) * 8, hipMemcpyDeviceToHost);
		if (e == hipSuccess && bytes)
			e = hipMemcpy(gather->outText, dOutText, size_t(bytes), hipMemcpyDeviceToHost);
		return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, backLabel);
	}
};

int RunLinesImpl(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, const uint64_t* want,
                 uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans, uint64_t* out_hit_masks, uint64_t hit_cap,
                 uint64_t* out_hit_count, void* streamPtr, const LinesGather* gather, const LinesField* column = nullptr)
{
	const char* who = column ? (gather ? "pire_hip_run_lines_field_gather" : "pire_hip_run_lines_field_select")
	                         : (gather ? "pire_hip_run_lines_gather" : "pire_hip_run_lines_select");
	// (the gather form keeps the hit list to itself where the caller has no array for it)
	if (int rc = SelectArgsInvalid(t, nullptr, false, 0, out_hits, out_hit_masks, gather && !out_hits ? 0 : hit_cap, out_hit_count))
		return rc;
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	if (out_hit_spans && !out_hits) {
		SetError("pire_hip_run_lines_select: out_hit_spans without out_hits");
		return PIRE_HIP_EINVAL;
	}
	if (column) {
		if (int rc = FieldArgsInvalid(who, column->sep, column->mode))
			return rc;
		if (column->sep == delim)
			return GatherRefuse(who, "sep == delim");
	}
	if (gather) {
		if (int rc = GatherOutputsInvalid(who, "hit_cap", hit_cap, gather->tail, gather->outText, gather->textCap, gather->outOffsets,
		                                  gather->outBytes))
			return rc;
		if (int rc = GatherOverlaps(who, raw, size, gather->outText, gather->textCap))
			return rc;
	}
	LinesFrame f(who, raw, size, delim, flags, gather, streamPtr);
	if (f.HostEdge(out_line_count)) {
		*out_hit_count = 0;
		return PIRE_HIP_OK;
	}
	const uint32_t words = pire_hip_table_mask_words(t);
	const uint64_t* dWant = nullptr;
	uint64_t* dHitMasks = nullptr;
	if (int rc = f.Open())
		return rc;
	if (want)
		if (int rc = f.io.In(want, size_t(words), &dWant))
			return rc;
	if (int rc = f.Split(out_line_count, out_hit_count, 1, hit_cap, true))
		return rc;
	if (int rc = f.Lists(out_hits, out_hit_spans))
		return rc;
	if (out_hits && out_hit_masks && f.cap)
		if (int rc = f.io.Result(out_hit_masks, size_t(f.cap) * words, 0, &dHitMasks))
			return rc;
	if (f.n == 0) {
		if (int rc = f.ZeroCounts("hipMemsetAsync(hit count)"))
			return rc;
	} else {
		if (column)
			if (int rc = f.Cut(*column))
				return rc;
		if (int rc = pire_hip_run_select(t, f.Text(), f.Offsets(), f.n, f.RunFlags(), nullptr, nullptr, nullptr, nullptr, dWant, nullptr,
		                                 f.dHits, dHitMasks, f.dHits ? f.cap : 0, f.dCounts, f.stream))
			return rc;
		if (f.dSpans)   // (the whole line, whatever part of it was scanned)
			if (int rc = LaunchHitSpans(f.dHits, f.dCounts, 1, f.cap, f.cap, f.LineOffsets(), f.dSpans, f.stream, "split spans launch"))
				return rc;
	}
	if (int rc = f.Close("hipMemcpy(hits)"))
		return rc;
	return f.onDevice ? PIRE_HIP_OK : HitsBack(1, out_hit_count, f.cap, f.cap, dHitMasks, out_hit_masks, size_t(words) * 8, "hipMemcpy(hits)");
}

// Both gather entry points behind their checks.  spans == nullptr: text + offsets[n + 1] + idx; else raw = text, `size` bytes.
int GatherImpl(const char* who, const void* text, const uint64_t* offsets, uint64_t n, const uint64_t* idx, const uint64_t* spans,
               uint64_t size, const uint64_t* count, uint64_t cap, uint32_t tail, uint32_t flags, void* outText, uint64_t textCap,
               uint64_t* outOffsets, uint64_t* outBytes, void* streamPtr)
{
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	if (flags & PIRE_HIP_RUN_ON_DEVICE) {
		const GatherSource src = {static_cast<const uint8_t*>(text), offsets, n, idx, spans, size};
		return LaunchGather(src, count, cap, tail, outText, textCap, outOffsets, outBytes, kGatherTotalUnknown, stream);
	}
	// the host's own look at what it is asked to copy: total = the bytes of the k strings and their tails (offsets that
	// decrease make it meaningless -- BatchIO::Text refuses them below, before anything is written)
	const uint64_t k = std::min(count ? *count : cap, cap);
	uint64_t total = tail != PIRE_HIP_GATHER_NO_TAIL ? k : 0;
	if (spans) {
		for (uint64_t j = 0; j < k; ++j) {
			if (spans[2 * j] > spans[2 * j + 1] || spans[2 * j + 1] > size)
				return GatherRefuse(who, "span out of range");
			total += spans[2 * j + 1] - spans[2 * j];
		}
	} else {
		for (uint64_t j = 0; j < k; ++j) {
			const uint64_t s = idx ? idx[j] : j;
			if (s >= n)
				return GatherRefuse(who, "index out of range");
			total += offsets[s + 1] - offsets[s];
		}
		if (k)
			if (int rc = GatherOverlaps(who, text, offsets[n], outText, textCap))
				return rc;
	}
	if (k == 0) {
		*outBytes = 0;
		if (outOffsets)
			outOffsets[0] = 0;
		return PIRE_HIP_OK;
	}
	BatchIO io(stream, false);
	GatherSource src = {nullptr, nullptr, n, nullptr, nullptr, size};
	if (spans) {
		if (int rc = io.In(static_cast<const uint8_t*>(text), size_t(size), &src.text))
			return rc;
		if (int rc = io.In(spans, size_t(k) * 2, &src.spans))
			return rc;
	} else {
		if (int rc = io.Text(text, offsets, n, 0, 0, &src.text, &src.offsets))
			return rc;
		if (idx)
			if (int rc = io.In(idx, size_t(k), &src.idx))
				return rc;
	}
	uint64_t *dBytes = nullptr, *dOutOffsets = nullptr;
	uint8_t* dOutText = nullptr;
	const uint64_t room = std::min(total, textCap);
	if (int rc = io.Result(outBytes, 1, 1, &dBytes))
		return rc;
	if (int rc = io.Result(outOffsets, size_t(k) + 1, size_t(k) + 1, &dOutOffsets))
		return rc;
	if (room)
		if (int rc = io.Result(static_cast<uint8_t*>(outText), size_t(room), size_t(room), &dOutText))
			return rc;
	if (int rc = io.Ready())
		return rc;
	if (int rc = LaunchGather(src, nullptr, k, tail, dOutText, room, dOutOffsets, dBytes, total, stream))
		return rc;
	return io.Finish();
}

}  // namespace

int pire_hip_run_lines_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                              const uint64_t* want, uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans,
                              uint64_t* out_hit_masks, uint64_t hit_cap, uint64_t* out_hit_count, void* stream)
try {
	return RunLinesImpl(t, raw, size, delim, flags, want, out_line_count, out_hits, out_hit_spans, out_hit_masks, hit_cap,
	                    out_hit_count, stream, nullptr);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// The frame around the route pass: the scan on the lines with the state indices in scratch, one hit list per regexp, and the
// byte ranges of all rows in one launch
int pire_hip_run_lines_route(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                             uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans, uint64_t hit_cap,
                             uint64_t* out_hit_counts, void* streamPtr)
try {
	const char* who = "pire_hip_run_lines_route";
	if (int rc = RouteArgsInvalid(who, t, nullptr, false, 0, out_hits, out_hit_spans, hit_cap, out_hit_counts))
		return rc;
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	const uint32_t regexps = HostRegexps(t);
	LinesFrame f(who, raw, size, delim, flags, nullptr, streamPtr);
	if (f.HostEdge(out_line_count)) {
		std::fill(out_hit_counts, out_hit_counts + regexps, uint64_t(0));
		return PIRE_HIP_OK;
	}
	if (int rc = f.Open())
		return rc;
	// (host pointers: n lines have at most n hits a row; a device caller's pitch is hit_cap itself)
	if (int rc = f.Split(out_line_count, out_hit_counts, regexps, hit_cap, !f.onDevice))
		return rc;
	if (int rc = f.Lists(out_hits, out_hit_spans))
		return rc;
	if (f.n == 0) {
		if (int rc = f.ZeroCounts("hipMemsetAsync(hit counts)"))
			return rc;
	} else if (regexps) {
		if (int rc = pire_hip_run_route(t, f.Text(), f.Offsets(), f.n, f.RunFlags(), nullptr, nullptr, nullptr, nullptr, f.dHits,
		                                f.dHits ? f.cap : 0, f.dCounts, f.stream))
			return rc;
		if (f.dSpans)   // (n lines: no row has more hits)
			if (int rc = LaunchHitSpans(f.dHits, f.dCounts, regexps, f.cap, std::min(f.cap, f.n), f.Offsets(), f.dSpans, f.stream,
			                            "route spans launch"))
				return rc;
	}
	return f.Close("hipMemcpy(route hits)");
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- the selected strings gathered into a batch (gather.hip) -------------------------------------------------------------
int pire_hip_gather(const void* text, const uint64_t* offsets, uint64_t n, const uint64_t* idx, const uint64_t* idx_count,
                    uint64_t idx_cap, uint32_t tail, uint32_t flags, void* out_text, uint64_t text_cap, uint64_t* out_offsets,
                    uint64_t* out_bytes, void* stream)
try {
	const char* who = "pire_hip_gather";
	if (int rc = GatherOutputsInvalid(who, nullptr, idx_cap, tail, out_text, text_cap, out_offsets, out_bytes))
		return rc;
	if (idx_cap && !offsets)
		return GatherRefuse(who, "idx_cap > 0 with null offsets");
	if (idx_cap > n && !idx)
		return GatherRefuse(who, "idx_cap > n without idx");
	if (idx_cap >= (1ull << 32))
		return GatherRefuse(who, "2^32 strings or more in one call");
	return GatherImpl(who, text, offsets, n, idx, nullptr, 0, idx_count, idx_cap, tail, flags, out_text, text_cap, out_offsets,
	                  out_bytes, stream);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_gather_spans(const void* raw, uint64_t size, const uint64_t* spans, const uint64_t* span_count, uint64_t span_cap,
                          uint32_t tail, uint32_t flags, void* out_text, uint64_t text_cap, uint64_t* out_offsets,
                          uint64_t* out_bytes, void* stream)
try {
	const char* who = "pire_hip_gather_spans";
	if (int rc = GatherOutputsInvalid(who, "span_cap", span_cap, tail, out_text, text_cap, out_offsets, out_bytes))
		return rc;
	if (span_cap && !spans)
		return GatherRefuse(who, "span_cap > 0 with null spans");
	if (span_cap >= (1ull << 32))
		return GatherRefuse(who, "2^32 strings or more in one call");
	if (int rc = GatherOverlaps(who, raw, size, out_text, text_cap))
		return rc;
	return GatherImpl(who, raw, nullptr, 0, nullptr, spans, size, span_count, span_cap, tail, flags, out_text, text_cap,
	                  out_offsets, out_bytes, stream);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_run_lines_gather(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                              const uint64_t* want, uint32_t tail, uint64_t* out_line_count, uint64_t* out_hits, uint64_t hit_cap,
                              uint64_t* out_hit_count, void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes,
                              void* stream)
try {
	const LinesGather gather = {tail, out_text, text_cap, out_offsets, out_bytes, true, "hipMallocAsync(hit spans)"};
	return RunLinesImpl(t, raw, size, delim, flags, want, out_line_count, out_hits, nullptr, nullptr, hit_cap, out_hit_count, stream,
	                    &gather);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- one column of every string (fields.hip) -------------------------------------------------------------------------------
int pire_hip_fields(const void* text, const uint64_t* offsets, uint64_t n, uint32_t sep, uint32_t field, uint32_t mode,
                    uint32_t flags, uint64_t* out_spans, void* streamPtr)
try {
	const char* who = "pire_hip_fields";
	if (int rc = FieldArgsInvalid(who, sep, mode))
		return rc;
	if (n && !offsets)
		return GatherRefuse(who, "n > 0 with null offsets");
	if (n && !out_spans)
		return GatherRefuse(who, "n > 0 with null out_spans");
	if (n >= (1ull << 32)) {
		SetError("pire_hip_fields: 2^32 strings or more in one call");
		return PIRE_HIP_EUNSUPPORTED;
	}
	if (n == 0)
		return PIRE_HIP_OK;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	if (!onDevice) {
		uint64_t textBytes = 0;
		if (int rc = CheckHostBatch(text, offsets, n, 0, 0, &textBytes))
			return rc;
	}
	BatchIO io(stream, onDevice);
	const uint8_t* dText = nullptr;
	const uint64_t* dOffsets = nullptr;
	uint64_t* dSpans = nullptr;
	if (int rc = io.Text(text, offsets, n, 0, 0, &dText, &dOffsets))
		return rc;
	if (int rc = io.Result(out_spans, size_t(n) * 2, size_t(n) * 2, &dSpans))
		return rc;
	if (int rc = io.Ready())
		return rc;
	if (int rc = LaunchFields(dText, dOffsets, n, sep, field, mode, dSpans, onDevice ? kFieldsBytesUnknown : offsets[n] - offsets[0], stream))
		return rc;
	return io.Finish();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_run_lines_field_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t sep, uint32_t field,
                                    uint32_t mode, uint32_t flags, const uint64_t* want, uint64_t* out_line_count, uint64_t* out_hits,
                                    uint64_t* out_hit_spans, uint64_t* out_hit_masks, uint64_t hit_cap, uint64_t* out_hit_count,
                                    void* stream)
try {
	const LinesField column = {sep, field, mode};
	return RunLinesImpl(t, raw, size, delim, flags, want, out_line_count, out_hits, out_hit_spans, out_hit_masks, hit_cap,
	                    out_hit_count, stream, nullptr, &column);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_run_lines_field_gather(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t sep, uint32_t field,
                                    uint32_t mode, uint32_t flags, const uint64_t* want, uint32_t tail, uint64_t* out_line_count,
                                    uint64_t* out_hits, uint64_t hit_cap, uint64_t* out_hit_count, void* out_text, uint64_t text_cap,
                                    uint64_t* out_offsets, uint64_t* out_bytes, void* stream)
try {
	const LinesGather gather = {tail, out_text, text_cap, out_offsets, out_bytes, true, "hipMallocAsync(hit spans)"};
	const LinesField column = {sep, field, mode};
	return RunLinesImpl(t, raw, size, delim, flags, want, out_line_count, out_hits, nullptr, nullptr, hit_cap, out_hit_count, stream,
	                    &gather, &column);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- raw bytes in, the captured field of every line out (split.hip, counting.hip, capture_select.hip, gather.hip) ---------
// The frame around a capturing scanner: the capture scan on the lines, the pass with shift = 1 (string i of the split buffer
// lies i bytes further into raw), the gather from raw through its spans.
int pire_hip_capture_lines_gather(pire_hip_counting_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                  int need_final, uint32_t tail, uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_spans,
                                  uint64_t hit_cap, uint64_t* out_hit_count, void* out_text, uint64_t text_cap,
                                  uint64_t* out_offsets, uint64_t* out_bytes, void* streamPtr)
try {
	const char* who = "pire_hip_capture_lines_gather";
	if (!t)
		return GatherRefuse(who, "null table");
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	// no gather output at all: spans only.  (The gather form keeps the span list to itself where the caller has no array for it.)
	const bool gathers = out_text || text_cap || out_offsets || out_bytes;
	if (int rc = CaptureSelectOutputsInvalid(who, 0, need_final, true, out_hits || out_spans || gathers, hit_cap, out_hit_count))
		return rc;
	if (gathers) {
		if (int rc = GatherOutputsInvalid(who, "hit_cap", hit_cap, tail, out_text, text_cap, out_offsets, out_bytes))
			return rc;
		if (int rc = GatherOverlaps(who, raw, size, out_text, text_cap))
			return rc;
	}
	const LinesGather gather = {tail, out_text, text_cap, out_offsets, out_bytes, false, "hipMallocAsync(capture spans)"};
	LinesFrame f(who, raw, size, delim, flags, gathers ? &gather : nullptr, streamPtr);
	if (f.HostEdge(out_line_count)) {
		*out_hit_count = 0;
		return PIRE_HIP_OK;
	}
	if (int rc = f.Open())
		return rc;
	if (int rc = f.Split(out_line_count, out_hit_count, 1, hit_cap, true))
		return rc;
	if (int rc = f.Lists(out_hits, out_spans))
		return rc;
	// (no lines: the pass itself zeroes the count)
	const CaptureSelectOut sel = {need_final, 1, f.dHits, f.dSpans, f.cap, f.dCounts};
	if (int rc = CaptureRunImpl(t, f.Text(), f.Offsets(), f.n, f.RunFlags(), nullptr, nullptr, nullptr, nullptr, &sel, f.stream))
		return rc;
	return f.Close("hipMemcpy(captures)");
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- the same two forms around a SlowCapturingScanner (slow_capture.hip): the pass reads the captured flags as Final ------
int pire_hip_slow_capture_run_select(pire_hip_slow_capture_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                                     uint8_t* out_captured, int64_t* out_begin, int64_t* out_end, uint8_t* out_matched, uint64_t* out_hits,
                                     uint64_t* out_spans, uint64_t hit_cap, uint64_t* out_hit_count, void* stream)
try {
	const char* who = "pire_hip_slow_capture_run_select";
	if (int rc = CaptureSelectOutputsInvalid(who, n, 1, true, out_hits || out_spans, hit_cap, out_hit_count))
		return rc;
	const CaptureSelectOut sel = {1, 0, out_hits, out_spans, hit_cap, out_hit_count};
	return SlowCaptureRunImpl(who, t, text, offsets, n, flags, out_captured, out_begin, out_end, out_matched, &sel, static_cast<hipStream_t>(stream));
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_slow_capture_lines_gather(pire_hip_slow_capture_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                       uint32_t tail, uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap,
                                       uint64_t* out_hit_count, void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes,
                                       void* streamPtr)
try {
	const char* who = "pire_hip_slow_capture_lines_gather";
	if (!t)
		return GatherRefuse(who, "null table");
	if (flags & (PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END))
		return GatherRefuse(who, "PIRE_HIP_RUN_BEGIN / PIRE_HIP_RUN_END: the scanner takes both marks itself");
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	const bool gathers = out_text || text_cap || out_offsets || out_bytes;
	if (int rc = CaptureSelectOutputsInvalid(who, 0, 1, true, out_hits || out_spans || gathers, hit_cap, out_hit_count))
		return rc;
	if (gathers) {
		if (int rc = GatherOutputsInvalid(who, "hit_cap", hit_cap, tail, out_text, text_cap, out_offsets, out_bytes))
			return rc;
		if (int rc = GatherOverlaps(who, raw, size, out_text, text_cap))
			return rc;
	}
	const LinesGather gather = {tail, out_text, text_cap, out_offsets, out_bytes, false, "hipMallocAsync(capture spans)"};
	LinesFrame f(who, raw, size, delim, flags, gathers ? &gather : nullptr, streamPtr);
	if (f.HostEdge(out_line_count)) {
		*out_hit_count = 0;
		return PIRE_HIP_OK;
	}
	if (int rc = f.Open())
		return rc;
	if (int rc = f.Split(out_line_count, out_hit_count, 1, hit_cap, true))
		return rc;
	if (int rc = f.Lists(out_hits, out_spans))
		return rc;
	// (no lines: the pass itself zeroes the count.  A line is a string of fewer than 2^32 - 1 bytes where the buffer is: the
	// split refuses 2^32 lines, not long ones -- a longer line is the precondition of the device form of the run call.)
	const CaptureSelectOut sel = {1, 1, f.dHits, f.dSpans, f.cap, f.dCounts};
	if (int rc = SlowCaptureRunImpl(who, t, f.Text(), f.Offsets(), f.n, f.RunFlags(), nullptr, nullptr, nullptr, nullptr, &sel, f.stream))
		return rc;
	return f.Close("hipMemcpy(captures)");
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- first-use self-tests of the entry points with actions (selftest.h) -------------------------------------------------
namespace {

enum : uint32_t { kEntryPrefix = 8, kEntrySuffix = 9, kEntryHalfFinal = 10, kEntryPair = 11 };   // bits of pire_hip_table::selfTested

// the table's transitions, flags and final lists in the reference's numbering: they never change (an adaptation renumbers
// the DEVICE side only)
struct HostWalk {
	const HostTable& h;
	uint32_t Next(uint32_t st, uint32_t ch) const { return h.next[size_t(st) * h.letters + h.cls[ch]]; }
	bool Final(uint32_t st) const { return (h.flags[st] & kFinal) != 0; }
	bool Dead(uint32_t st) const { return (h.flags[st] & kDead) != 0; }
	uint64_t Salt() const { return (uint64_t(h.states) << 20) ^ h.letters; }   // (KnownBatchFor)
};

// LongestPrefix / ShortestPrefix as the reference walks them (run.h:69-100, 277-311), on the host table
int64_t HostPrefix(const HostWalk& w, const uint8_t* b, const uint8_t* e, bool longest, bool throughBegin, bool throughEnd)
{
	uint32_t st = w.h.initial;
	if (throughBegin)
		st = w.Next(st, kBeginMark);
	int64_t pos = -1;
	if (longest) {
		if (w.Final(st))
			pos = 0;
		for (const uint8_t* p = b; p != e; ++p) {
			st = w.Next(st, *p);
			if (w.Final(st))
				pos = p + 1 - b;
			if (w.Dead(st))
				break;
		}
		if (throughEnd && w.Final(w.Next(st, kEndMark)))
			pos = e - b;
		return pos;
	}
	if (w.Final(st))
		return 0;
	for (const uint8_t* p = b; p != e; ++p) {
		st = w.Next(st, *p);
		if (w.Final(st))
			return p + 1 - b;
		if (w.Dead(st))
			break;
	}
	if (throughEnd && w.Final(w.Next(st, kEndMark)))
		return e - b;
	return -1;
}

// LongestSuffix / ShortestSuffix (run.h:313-362): backwards from the last byte
int64_t HostSuffix(const HostWalk& w, const uint8_t* first, const uint8_t* last1, bool longest, bool throughEnd, bool throughBegin)
{
	uint32_t st = w.h.initial;
	if (throughEnd)
		st = w.Next(st, kEndMark);
	const uint8_t* r = last1;   // one past the byte the walk takes next (going down)
	if (longest) {
		int64_t pos = -1;
		while (r != first && !w.Dead(st)) {
			if (w.Final(st))
				pos = last1 - r;
			st = w.Next(st, r[-1]);
			--r;
		}
		if (w.Final(st))
			pos = last1 - r;
		if (throughBegin && w.Final(w.Next(st, kBeginMark)))
			pos = last1 - r;
		return pos;
	}
	for (; r != first && !w.Final(st) && !w.Dead(st); --r)
		st = w.Next(st, r[-1]);
	if (throughBegin)
		st = w.Next(st, kBeginMark);
	return w.Final(st) ? int64_t(last1 - r) : -1;
}

// Marks an entry point tested on this device -- unless a re-ranking has meanwhile zipped the wide image or given the plain rows
// back (it cleared the bit: ForgetLayoutSelfTests), so that the next call tests the other instantiations.
void MarkEntryTested(pire_hip_table* t, int dev, uint32_t bit, bool zipped)
{
	std::shared_lock<std::shared_mutex> stable(t->adaptMutex);
	if ((t->host.zipFull != 0) == zipped)
		MarkTested(t, dev, bit);
}

int SelfTestPrefix(pire_hip_table* t, bool suffix, int a, int b, hipStream_t stream)
{
	uint32_t mode = 0;
	int dev = -1;
	const uint32_t bit = suffix ? kEntrySuffix : kEntryPrefix;
	if (EntryTested(t, bit, &dev))
		return PIRE_HIP_OK;
	// The known batch, its answers and the variants come from the host table under adaptMutex SHARED (a background swap replaces
	// t->host) and the table's configuration; the lock is released before the variants call the entry point, which takes it again.
	TableConfigScope scope;
	std::shared_lock<std::shared_mutex> stable(t->adaptMutex);
	scope.Push(t);
	if (t->host.empty || !EntrySelfTestDue(stream, &mode))
		return PIRE_HIP_OK;
	const bool zipped = t->host.zipFull != 0;
	const HostWalk w{t->host};
	// (prefix: a = throughBegin, b = throughEnd; suffix: a = throughEnd, b = throughBegin -- the mark the walk starts with first)
	const uint32_t start = a ? w.Next(t->host.initial, suffix ? kEndMark : kBeginMark) : t->host.initial;
	const KnownBatch kb = KnownBatchFor(w, start, suffix ? 2 : 1);
	std::vector<int64_t> wants[2];
	for (int longest = 0; longest < 2; ++longest) {
		std::vector<int64_t>& want = wants[longest];
		want.resize(kb.n);
		for (uint32_t i = 0; i < kb.n; ++i) {
			const uint8_t* s0 = kb.text.data() + kb.offsets[i];
			const uint8_t* s1 = kb.text.data() + kb.offsets[i + 1];
			want[i] = suffix ? HostSuffix(w, s0, s1, longest != 0, a != 0, b != 0) : HostPrefix(w, s0, s1, longest != 0, a != 0, b != 0);
		}
		if (mode == 2)
			want[kb.n / 2] += 1;
	}
	std::vector<ConfigEdit> variants;
	variants.push_back([](pire_hip_config& c) { c.ragged_act_always = 1; c.no_ragged_act = 0; });   // the ragged kernel with actions
	if (!suffix)
		variants.push_back([](pire_hip_config& c) { c.no_ragged_act = 1; c.ragged_act_always = 0; });   // one string per lane
	if (!suffix && t->host.wide && t->host.states <= 65536)   // ... and the ragged kernel with actions on the class-indexed walk
		variants.push_back([](pire_hip_config& c) { c.ragged_act_always = 1; c.no_ragged_act = 0; c.walk_variant = 2; c.tiled_variant = 0; c.checked = 0; });
	stable.unlock();
	for (int longest = 0; longest < 2; ++longest) {
		const std::vector<int64_t>& want = wants[longest];
		std::vector<int64_t> got(kb.n);
		const int rc = RunKnownAnswer(variants, [&] { std::fill(got.begin(), got.end(), int64_t(-77)); }, [&](hipStream_t own) {
			return suffix ? pire_hip_suffix(t, kb.text.data(), kb.offsets.data(), kb.n, longest, a, b, 0, got.data(), own)
			              : pire_hip_prefix(t, kb.text.data(), kb.offsets.data(), kb.n, longest, a, b, 0, got.data(), own);
		}, [&]() -> int {
			for (uint32_t i = 0; i < kb.n; ++i)
				if (got[i] != want[i])
					return SelfTestMismatch(suffix ? (longest ? "LongestSuffix" : "ShortestSuffix") : (longest ? "LongestPrefix" : "ShortestPrefix"),
					                        i, std::to_string(got[i]), std::to_string(want[i]));
			return PIRE_HIP_OK;
		});
		if (rc != PIRE_HIP_OK)
			return rc;
	}
	MarkEntryTested(t, dev, bit, zipped);
	return PIRE_HIP_OK;
}

// HalfFinalScanner (half_final.h:137-164): Initialize and every Step end with TakeAction
int SelfTestHalfFinal(pire_hip_table* t, uint32_t flags, hipStream_t stream)
{
	uint32_t mode = 0;
	int dev = -1;
	if (EntryTested(t, kEntryHalfFinal, &dev))
		return PIRE_HIP_OK;
	TableConfigScope scope;   // (as SelfTestPrefix: the host table under the lock, released before the entry point is called)
	std::shared_lock<std::shared_mutex> stable(t->adaptMutex);
	scope.Push(t);
	if (t->host.empty || !EntrySelfTestDue(stream, &mode))
		return PIRE_HIP_OK;
	const bool zipped = t->host.zipFull != 0;
	const HostTable& h = t->host;
	const HostWalk w{h};
	const uint32_t R = h.regexps;
	flags &= PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END;
	const uint32_t start = (flags & PIRE_HIP_RUN_BEGIN) ? w.Next(h.initial, kBeginMark) : h.initial;
	const KnownBatch kb = KnownBatchFor(w, start, 3);
	std::vector<uint32_t> wantIdx(kb.n), wantRes(size_t(kb.n) * R, 0), gotIdx(kb.n), gotRes(size_t(kb.n) * R);
	std::vector<uint8_t> wantFin(kb.n), gotFin(kb.n);
	for (uint32_t i = 0; i < kb.n; ++i) {
		uint32_t* m = wantRes.data() + size_t(i) * R;
		auto take = [&](uint32_t st) {
			if (w.Final(st))
				for (uint64_t k = h.acceptOff[st]; k < h.acceptOff[st + 1]; ++k)
					m[h.acceptIds[k]]++;
		};
		uint32_t st = h.initial;
		take(st);
		if (flags & PIRE_HIP_RUN_BEGIN)
			take(st = w.Next(st, kBeginMark));
		for (uint64_t k = kb.offsets[i]; k < kb.offsets[i + 1]; ++k)
			take(st = w.Next(st, kb.text[k]));
		if (flags & PIRE_HIP_RUN_END)
			take(st = w.Next(st, kEndMark));
		wantIdx[i] = st;
		wantFin[i] = w.Final(st) ? 1 : 0;
	}
	if (mode == 2)
		wantIdx[kb.n / 2] ^= 1;
	std::vector<ConfigEdit> variants;
	variants.push_back([](pire_hip_config& c) { c.counting_variant = 2; });                        // the row kernel where the table has that image
	variants.push_back([](pire_hip_config& c) { c.counting_variant = 1; c.no_ragged_act = 0; });   // the ragged kernel with actions
	variants.push_back([](pire_hip_config& c) { c.counting_variant = 1; c.no_ragged_act = 1; });   // one string per lane
	if (h.wide && h.states <= 65536)   // the ragged kernel with actions on the class-indexed walk
		variants.push_back([](pire_hip_config& c) { c.counting_variant = 1; c.no_ragged_act = 0; c.walk_variant = 2; c.tiled_variant = 0; c.checked = 0; });
	stable.unlock();
	const int rc = RunKnownAnswer(variants, [&] {
		std::fill(gotIdx.begin(), gotIdx.end(), ~0u);
		std::fill(gotRes.begin(), gotRes.end(), ~0u);
	}, [&](hipStream_t own) {
		return pire_hip_run_half_final(t, kb.text.data(), kb.offsets.data(), kb.n, flags, gotIdx.data(), gotFin.data(), gotRes.data(), own);
	}, [&]() -> int {
		for (uint32_t i = 0; i < kb.n; ++i) {
			if (gotIdx[i] != wantIdx[i] || gotFin[i] != wantFin[i])
				return SelfTestMismatch("HalfFinalScanner", i, "state " + std::to_string(gotIdx[i]), "state " + std::to_string(wantIdx[i]));
			for (uint32_t r2 = 0; r2 < R; ++r2)
				if (gotRes[size_t(i) * R + r2] != wantRes[size_t(i) * R + r2])
					return SelfTestMismatch("HalfFinalScanner", i, "count " + std::to_string(gotRes[size_t(i) * R + r2]) + " for regexp " + std::to_string(r2),
					                        std::to_string(wantRes[size_t(i) * R + r2]));
		}
		return PIRE_HIP_OK;
	});
	if (rc != PIRE_HIP_OK)
		return rc;
	MarkEntryTested(t, dev, kEntryHalfFinal, zipped);
	return PIRE_HIP_OK;
}

// sel == nullptr: pire_hip_run_half_final.  Else out_results may be null, and the pass of count_select.hip follows the scan on
// the same stream, whichever way the counts were taken (pire_hip_run_half_final_select, pire_hip_half_final_lines_select).
int HalfFinalRunImpl(const char* who, pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                     uint32_t* out_state_idx, uint8_t* out_final, uint32_t* out_results, const CountSelectOut* sel, hipStream_t stream)
{
	if (!t || (n && (!offsets || (!sel && !out_results)))) {
		SetError(sel ? std::string(who) + ": null argument" : std::string("null argument"));
		return PIRE_HIP_EINVAL;
	}
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	std::optional<CountSelectStage> pass;
	if (sel) {
		const uint32_t regexps = HostRegexps(t);
		if (int rc = CountSelectArgsInvalid(who, n, regexps, true, *sel))
			return rc;
		pass.emplace(*sel, regexps, onDevice);
		if (n == 0)
			return pass->Empty(stream);
	}
	if (n)
		if (int rc = SelfTestHalfFinal(t, flags, stream))   // first use on this device: every kernel of this entry point, known answers
			return rc;
	ScanParams p;
	const bool enqueueOnly = (flags & PIRE_HIP_RUN_ON_DEVICE) && !(flags & PIRE_HIP_RUN_HOST_OFFSETS);
	TableUse use(t, enqueueOnly);
	if (int rc = FillParams(t, &p, 0, /*wantDist=*/true))   // startPerm = Initialize(); Begin() is a counted step in the kernel
		return rc;
	p.flags = flags & (PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END);
	p.n = n;
	if (n == 0)
		return PIRE_HIP_OK;
	const uint32_t R = t->host.regexps;
	p.actDist = p.distFinalPerm;
	{   // Initialize() and Begin() of a HalfFinalScanner end with TakeAction: walked once here (ScanParams::hfStart)
		const HostTable& h = t->host;
		uint32_t o = h.initial;
		auto take = [&](uint32_t st) {
			if ((h.flags[st] & kFinal) && h.incPacked)
				for (int r = 0; r < 8; ++r)
					p.hfStartC[r] += uint32_t(h.inc64[st] >> (8 * r)) & 0xFFu;
		};
		take(o);
		if (flags & PIRE_HIP_RUN_BEGIN) {
			o = h.next[size_t(o) * h.letters + h.cls[kBeginMark]];
			take(o);
		}
		p.hfStart = p.hostPermOfOrig[o];   // the numbering of the image in p (FillParams), not whatever t->host holds by now
	}
	// PIRE_HIP_RUN_GENERIC keeps the one-string-per-lane kernel (tests compare the two)
	const bool exactOnly = (flags & PIRE_HIP_RUN_GENERIC) != 0;
	// few long strings: the segmented scan resolves every segment's true start state, then the segments are counted
	// in parallel (segmented.hip); needs the lengths on the host and counters that pack.  false: not done.
	auto segmented = [&](const uint64_t* hostOffsets, uint32_t* dResults, bool* done) -> int {
		*done = false;
		if (exactOnly || !p.incPerm || !SegmentedEligible(n, hostOffsets[n] - hostOffsets[0]))
			return PIRE_HIP_OK;
		ScanParams ps;
		if (int rc = FillParams(t, &ps, flags & (PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END)))   // Begin() folded into the start; the same image as p (`use`)
			return rc;
		ps.n = n;
		ps.text = p.text;
		ps.offsets = p.offsets;
		ps.outIdx = p.outIdx;
		ps.outFinal = p.outFinal;
		bool incomplete = false;
		if (int rc = RunSegmented(t, ps, hostOffsets, stream, dResults, &incomplete))
			return rc;
		*done = !incomplete;
		return PIRE_HIP_OK;
	};
	// Scanners whose walk is in a Final state most of the time gain nothing from the ragged kernel's look for the chunks
	// that hold one: those take the row kernel of the counting scanners (counting.hip: whole text lines per lane, the
	// increments of the target state as the step's action), and what its 16-bit counters cannot hold -- strings of more
	// than 65 000 bytes -- the one-string-per-lane kernel, from the list the row kernel leaves.
	auto launchCounting = [&](uint32_t* dResults) -> int {
		// (the share of the byte model's visits that fall on Final states decides, as for the capturing scanners: at 0.2 %
		// of the steps a third of the ragged kernel's chunks are walked again)
		if (!exactOnly && (!RaggedActEligible(p) || p.finalShare > 0.002f)) {
			bool done = false;
			StreamScratch list(stream);   // the strings the row kernel left: alive until the kernel that counts them is enqueued
			if (int rc = LaunchHalfFinalRows(t, p.text, p.offsets, n, flags, p.outIdx, p.outFinal, dResults, stream, &done, &list))
				return rc;
			if (done)
				return LaunchHalfFinal(p, dResults, stream, nullptr, list.as<uint32_t>());
		}
		return LaunchHalfFinal(p, dResults, stream, exactOnly ? nullptr : NextWorkSlot(t, p));
	};
	BatchIO io(stream, onDevice);
	uint32_t* dRes = nullptr;
	int rc;
	if ((rc = io.Text(text, offsets, n, 0, 0, &p.text, &p.offsets)) || (pass && (rc = pass->In(io))) ||
	    (rc = io.Result(out_state_idx, size_t(n), size_t(n), &p.outIdx)) || (rc = io.Result(out_final, size_t(n), size_t(n), &p.outFinal)) ||
	    (rc = io.Result(out_results, size_t(n) * std::max<uint32_t>(R, 1), size_t(n) * R, &dRes)))
		return rc;
	// the pass behind the scan: the rows it reads and the caller has no array for live in scratch (a host-pointer call's
	// Result() has allocated them already)
	StreamScratch ownResults(stream);
	if (pass) {
		if (!dRes) {
			if ((rc = ownResults.Alloc(size_t(n) * std::max<uint32_t>(R, 1) * 4, "hipMallocAsync(half-final results)")))
				return rc;
			dRes = ownResults.as<uint32_t>();
		}
		if ((rc = pass->Results(io, n)))
			return rc;
	}
	if ((rc = io.Ready()))
		return rc;
	// the lengths on the host (its own arrays, or PIRE_HIP_RUN_HOST_OFFSETS: resident text, see pire_hip_run): the
	// segmented scan first
	const bool hostOffsets = !enqueueOnly;
	auto count = [&]() -> int {
		bool counted = false;
		if (hostOffsets)
			if (int src = segmented(offsets, dRes, &counted))
				return src;
		return counted ? PIRE_HIP_OK : launchCounting(dRes);
	};
	if (onDevice && hostOffsets)
		rc = WithOffsetsOnDevice(offsets, n, stream, [&](const uint64_t* dOffsets) {
			p.offsets = dOffsets;
			return count();
		});
	else
		rc = count();
	if (rc || (pass && (rc = pass->Launch(dRes, n, stream))) || (rc = io.Finish()))
		return rc;
	return pass ? pass->Back() : PIRE_HIP_OK;
}

}  // namespace

int pire_hip_run_half_final(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                            uint32_t* out_state_idx, uint8_t* out_final, uint32_t* out_results, void* stream)
try {
	return HalfFinalRunImpl("pire_hip_run_half_final", t, text, offsets, n, flags, out_state_idx, out_final, out_results, nullptr,
	                        static_cast<hipStream_t>(stream));
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_run_half_final_select(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                                   uint32_t* out_state_idx, uint8_t* out_final, uint32_t* out_results, const uint32_t* min_count,
                                   uint32_t mode, uint64_t* out_totals, uint64_t* out_hits, uint32_t* out_hit_results, uint64_t hit_cap,
                                   uint64_t* out_hit_count, void* stream)
try {
	const CountSelectOut sel = {min_count, mode, out_totals, out_hits, out_hit_results, hit_cap, out_hit_count};
	return HalfFinalRunImpl("pire_hip_run_half_final_select", t, text, offsets, n, flags, out_state_idx, out_final, out_results, &sel,
	                        static_cast<hipStream_t>(stream));
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- raw bytes in, the lines that count out (split.hip, counting.hip, count_select.hip) -------------------------------------
// The frame around a counting scan: the scan on the lines with the rows in scratch, the pass, the whole lines of the hits as
// byte ranges of raw.  `scan`: the run + pass call on device pointers (the line batch, the pass's arguments on the device).
namespace {

int CountLinesImpl(const char* who, uint32_t regexps, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, const CountSelectOut& o,
                   uint64_t* out_line_count, uint64_t* out_hit_spans, void* streamPtr,
                   const std::function<int(const LinesFrame&, const CountSelectOut&)>& scan)
{
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	if (int rc = CountSelectArgsInvalid(who, 0, regexps, true, o))
		return rc;
	if (out_hit_spans && !o.outHits) {
		SetError(std::string(who) + ": out_hit_spans without out_hits");
		return PIRE_HIP_EINVAL;
	}
	LinesFrame f(who, raw, size, delim, flags, nullptr, streamPtr);
	if (f.HostEdge(out_line_count))
		return CountSelectStage(o, regexps, false).Empty(f.stream);
	const uint32_t* dMin = o.minCount;
	uint64_t* dTotals = o.outTotals;
	uint32_t* dHitResults = nullptr;
	if (int rc = f.Open())
		return rc;
	if (o.minCount)
		if (int rc = f.io.In(o.minCount, size_t(regexps), &dMin))
			return rc;
	if (int rc = f.Split(out_line_count, o.outHitCount, 1, o.hitCap, true))
		return rc;
	if (int rc = f.Lists(o.outHits, out_hit_spans))
		return rc;
	if (o.outTotals && regexps)
		if (int rc = f.io.Result(o.outTotals, size_t(regexps), size_t(regexps), &dTotals))
			return rc;
	if (o.outHitResults && f.cap && regexps)
		if (int rc = f.io.Result(o.outHitResults, size_t(f.cap) * regexps, 0, &dHitResults))
			return rc;
	// (no lines: the pass itself zeroes the count and the totals)
	const CountSelectOut onLines = {dMin, o.mode, dTotals, f.dHits, dHitResults, f.dHits || dHitResults ? f.cap : 0, f.dCounts};
	if (int rc = scan(f, onLines))
		return rc;
	if (f.dSpans && f.n)   // (the whole line)
		if (int rc = LaunchHitSpans(f.dHits, f.dCounts, 1, f.cap, f.cap, f.LineOffsets(), f.dSpans, f.stream, "split spans launch"))
			return rc;
	if (int rc = f.Close("hipMemcpy(hits)"))
		return rc;
	return f.onDevice ? PIRE_HIP_OK : HitsBack(1, o.outHitCount, f.cap, f.cap, dHitResults, o.outHitResults, size_t(regexps) * 4, "hipMemcpy(hits)");
}

}  // namespace

int pire_hip_counting_lines_select(pire_hip_counting_table* t, int kind, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                   const uint32_t* min_count, uint32_t mode, uint64_t* out_line_count, uint64_t* out_totals,
                                   uint64_t* out_hits, uint64_t* out_hit_spans, uint32_t* out_hit_results, uint64_t hit_cap,
                                   uint64_t* out_hit_count, void* stream)
try {
	const char* who = "pire_hip_counting_lines_select";
	pire_hip_counting_info info;
	if (!t || pire_hip_counting_table_get_info(t, &info) != PIRE_HIP_OK)
		return GatherRefuse(who, "null table");
	const CountSelectOut o = {min_count, mode, out_totals, out_hits, out_hit_results, hit_cap, out_hit_count};
	return CountLinesImpl(who, info.regexps, raw, size, delim, flags, o, out_line_count, out_hit_spans, stream,
	                      [&](const LinesFrame& f, const CountSelectOut& onLines) {
		                      return CountingRunImpl(who, t, kind, f.Text(), f.Offsets(), f.n, f.RunFlags(), nullptr, nullptr, &onLines, f.stream);
	                      });
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_half_final_lines_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                     const uint32_t* min_count, uint32_t mode, uint64_t* out_line_count, uint64_t* out_totals,
                                     uint64_t* out_hits, uint64_t* out_hit_spans, uint32_t* out_hit_results, uint64_t hit_cap,
                                     uint64_t* out_hit_count, void* stream)
try {
	const char* who = "pire_hip_half_final_lines_select";
	if (!t)
		return GatherRefuse(who, "null table");
	const CountSelectOut o = {min_count, mode, out_totals, out_hits, out_hit_results, hit_cap, out_hit_count};
	return CountLinesImpl(who, HostRegexps(t), raw, size, delim, flags, o, out_line_count, out_hit_spans, stream,
	                      [&](const LinesFrame& f, const CountSelectOut& onLines) {
		                      return HalfFinalRunImpl(who, t, f.Text(), f.Offsets(), f.n, f.RunFlags(), nullptr, nullptr, nullptr, &onLines, f.stream);
	                      });
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- raw bytes in, the lines a SlowScanner matches -- or does not -- out (split.hip, slow.hip, slow_hits.hip) ----------------
// The frame around a SlowScanner's scan: the scan on the lines with the Final flags in scratch, the pass, the whole lines of
// the hits as byte ranges of raw and, in the gather form, their bytes.  The frame itself takes no table: the scan is the
// entry point's own call.
namespace {

int SlowLinesImpl(const char* who, pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint32_t mode,
                  uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans, uint64_t hit_cap, uint64_t* out_hit_count,
                  void* streamPtr, const LinesGather* gather)
{
	if (!t)
		return GatherRefuse(who, "null table");
	// (the gather form keeps the hit list to itself where the caller has no array for it)
	const FinalSelectOut o = {mode, out_hits, gather && !out_hits ? 0 : hit_cap, out_hit_count};
	if (int rc = FinalSelectArgsInvalid(who, 0, true, o))
		return rc;
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	if (out_hit_spans && !out_hits)
		return GatherRefuse(who, "out_hit_spans without out_hits");
	if (gather) {
		if (int rc = GatherOutputsInvalid(who, "hit_cap", hit_cap, gather->tail, gather->outText, gather->textCap, gather->outOffsets,
		                                  gather->outBytes))
			return rc;
		if (int rc = GatherOverlaps(who, raw, size, gather->outText, gather->textCap))
			return rc;
	}
	LinesFrame f(who, raw, size, delim, flags, gather, streamPtr);
	if (f.HostEdge(out_line_count)) {
		*out_hit_count = 0;
		return PIRE_HIP_OK;
	}
	if (int rc = f.Open())
		return rc;
	if (int rc = f.Split(out_line_count, out_hit_count, 1, hit_cap, true))
		return rc;
	if (int rc = f.Lists(out_hits, out_hit_spans))
		return rc;
	if (f.n == 0) {
		if (int rc = f.ZeroCounts("hipMemsetAsync(hit count)"))
			return rc;
	} else {
		if (int rc = pire_hip_slow_run_select(t, f.Text(), f.Offsets(), f.n, f.RunFlags(), mode, nullptr, nullptr, nullptr, f.dHits,
		                                      f.dHits ? f.cap : 0, f.dCounts, f.stream))
			return rc;
		if (f.dSpans)   // (the whole line)
			if (int rc = LaunchHitSpans(f.dHits, f.dCounts, 1, f.cap, f.cap, f.LineOffsets(), f.dSpans, f.stream, "split spans launch"))
				return rc;
	}
	return f.Close("hipMemcpy(hits)");
}

}  // namespace

int pire_hip_slow_lines_select(pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint32_t mode,
                               uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans, uint64_t hit_cap,
                               uint64_t* out_hit_count, void* stream)
try {
	return SlowLinesImpl("pire_hip_slow_lines_select", t, raw, size, delim, flags, mode, out_line_count, out_hits, out_hit_spans, hit_cap,
	                     out_hit_count, stream, nullptr);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_slow_lines_gather(pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint32_t mode,
                               uint32_t tail, uint64_t* out_line_count, uint64_t* out_hits, uint64_t hit_cap, uint64_t* out_hit_count,
                               void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* stream)
try {
	const LinesGather gather = {tail, out_text, text_cap, out_offsets, out_bytes, true, "hipMallocAsync(hit spans)"};
	return SlowLinesImpl("pire_hip_slow_lines_gather", t, raw, size, delim, flags, mode, out_line_count, out_hits, nullptr, hit_cap,
	                     out_hit_count, stream, &gather);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- raw bytes in, the lines that match and their neighbours out (split.hip, context.hip) ----------------------------------
// The frame around scan + hit list + pire_hip_context: the hit list of the scan lives in scratch, the context list takes the
// place the hit list has in the forms above -- lines, spans, the gather through the spans.  The frame takes no table: the
// scan is the entry point's own call (Scanner: with `want` staged in; SlowScanner: with `mode`).
namespace {

struct ContextLines {
	uint64_t before, after;
	uint64_t* outLines;
	uint8_t* outFlags;
	uint64_t* outSpans;
	uint64_t lineCap;
	uint64_t *outSelCount, *outGroupCount, *outHitCount;
};

// scan(f, dWant, dHits, dHitCount): the hit list of the lines f.Text() / f.Offsets() / f.n into dHits[f.n], their number into *dHitCount
int ContextLinesImpl(const char* who, const char* refused, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, const uint64_t* want,
                     uint32_t wantWords, const ContextLines& c, uint64_t* out_line_count, const LinesGather* gather, void* streamPtr,
                     const std::function<int(const LinesFrame&, const uint64_t*, uint64_t*, uint64_t*)>& scan)
{
	if (refused)
		return GatherRefuse(who, refused);
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	if (!c.outSelCount)
		return GatherRefuse(who, "null out_sel_count");
	// (the gather form keeps the line list to itself where the caller has no array for it)
	const ContextOut o = {c.outLines, c.outFlags, c.lineCap, c.outSelCount, c.outGroupCount};
	if (int rc = ContextArgsInvalid(who, true, 0, 0, o, gather != nullptr))
		return rc;
	if (c.outSpans && !c.outLines)
		return GatherRefuse(who, "out_line_spans without out_lines");
	if (gather) {
		if (int rc = GatherOutputsInvalid(who, "line_cap", c.lineCap, gather->tail, gather->outText, gather->textCap, gather->outOffsets,
		                                  gather->outBytes))
			return rc;
		if (int rc = GatherOverlaps(who, raw, size, gather->outText, gather->textCap))
			return rc;
	}
	LinesFrame f(who, raw, size, delim, flags, gather, streamPtr);
	if (f.HostEdge(out_line_count)) {
		*c.outSelCount = 0;
		if (c.outGroupCount)
			*c.outGroupCount = 0;
		if (c.outHitCount)
			*c.outHitCount = 0;
		return PIRE_HIP_OK;
	}
	const uint64_t* dWant = nullptr;
	uint8_t* dFlags = nullptr;
	uint64_t *dGroups = nullptr, *dHitCount = nullptr;
	if (int rc = f.Open())
		return rc;
	if (want)
		if (int rc = f.io.In(want, size_t(wantWords), &dWant))
			return rc;
	if (int rc = f.Split(out_line_count, c.outSelCount, 1, c.lineCap, true))
		return rc;
	if (int rc = f.Lists(c.outLines, c.outSpans))
		return rc;
	if (c.outFlags && f.cap)
		if (int rc = f.io.Result(c.outFlags, size_t(f.cap), 0, &dFlags))
			return rc;
	if (c.outGroupCount)
		if (int rc = f.io.Result(c.outGroupCount, 1, 1, &dGroups))
			return rc;
	if (c.outHitCount)
		if (int rc = f.io.Result(c.outHitCount, 1, 1, &dHitCount))
			return rc;
	StreamScratch hitList(f.stream);   // (lives until the pass behind the scan is enqueued)
	if (f.n == 0) {
		if (int rc = f.ZeroCounts("hipMemsetAsync(line count)"))
			return rc;
		hipError_t e = dGroups ? hipMemsetAsync(dGroups, 0, 8, f.stream) : hipSuccess;
		if (e == hipSuccess && dHitCount)
			e = hipMemsetAsync(dHitCount, 0, 8, f.stream);
		if (e != hipSuccess)
			return HipFail(e, "hipMemsetAsync(line count)");
	} else {
		// the scan's hit list: 8 bytes a line at most, and its count where the caller has no place for it
		if (int rc = hitList.Alloc((size_t(f.n) + 1) * 8, "hipMallocAsync(context hits)"))
			return rc;
		uint64_t* dScanHits = hitList.as<uint64_t>();
		if (!dHitCount)
			dHitCount = dScanHits + f.n;
		if (int rc = scan(f, dWant, dScanHits, dHitCount))
			return rc;
		if (int rc = LaunchContext(dScanHits, dHitCount, f.n, f.n, c.before, c.after, f.dHits, dFlags, f.dHits ? f.cap : 0, f.dCounts, dGroups,
		                           f.stream))
			return rc;
		if (f.dSpans)   // (the whole line)
			if (int rc = LaunchHitSpans(f.dHits, f.dCounts, 1, f.cap, f.cap, f.LineOffsets(), f.dSpans, f.stream, "split spans launch"))
				return rc;
	}
	if (int rc = f.Close("hipMemcpy(context lines)"))
		return rc;
	return f.onDevice ? PIRE_HIP_OK : HitsBack(1, c.outSelCount, f.cap, f.cap, dFlags, c.outFlags, 1, "hipMemcpy(context lines)");
}

int RunLinesContextImpl(const char* who, pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, const uint64_t* want,
                        const ContextLines& c, uint64_t* out_line_count, const LinesGather* gather, void* stream)
{
	return ContextLinesImpl(who, t ? nullptr : "null table", raw, size, delim, flags, want, t ? pire_hip_table_mask_words(t) : 0, c,
	                        out_line_count, gather, stream,
	                        [&](const LinesFrame& f, const uint64_t* dWant, uint64_t* dHits, uint64_t* dHitCount) {
		                        return pire_hip_run_select(t, f.Text(), f.Offsets(), f.n, f.RunFlags(), nullptr, nullptr, nullptr, nullptr, dWant,
		                                                   nullptr, dHits, nullptr, f.n, dHitCount, f.stream);
	                        });
}

int SlowLinesContextImpl(const char* who, pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint32_t mode,
                         const ContextLines& c, uint64_t* out_line_count, const LinesGather* gather, void* stream)
{
	return ContextLinesImpl(who, !t ? "null table" : mode > PIRE_HIP_FINAL_SELECT_ZERO ? "unknown mode" : nullptr, raw, size, delim, flags,
	                        nullptr, 0, c, out_line_count, gather, stream,
	                        [&](const LinesFrame& f, const uint64_t*, uint64_t* dHits, uint64_t* dHitCount) {
		                        return pire_hip_slow_run_select(t, f.Text(), f.Offsets(), f.n, f.RunFlags(), mode, nullptr, nullptr, nullptr, dHits,
		                                                        f.n, dHitCount, f.stream);
	                        });
}

}  // namespace

int pire_hip_run_lines_context_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, const uint64_t* want,
                                      uint64_t before, uint64_t after, uint64_t* out_line_count, uint64_t* out_lines, uint8_t* out_line_flags,
                                      uint64_t* out_line_spans, uint64_t line_cap, uint64_t* out_sel_count, uint64_t* out_group_count,
                                      uint64_t* out_hit_count, void* stream)
try {
	const ContextLines c = {before, after, out_lines, out_line_flags, out_line_spans, line_cap, out_sel_count, out_group_count, out_hit_count};
	return RunLinesContextImpl("pire_hip_run_lines_context_select", t, raw, size, delim, flags, want, c, out_line_count, nullptr, stream);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_run_lines_context_gather(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, const uint64_t* want,
                                      uint64_t before, uint64_t after, uint64_t* out_line_count, uint64_t* out_lines, uint8_t* out_line_flags,
                                      uint64_t* out_line_spans, uint64_t line_cap, uint64_t* out_sel_count, uint64_t* out_group_count,
                                      uint64_t* out_hit_count, uint32_t tail, void* out_text, uint64_t text_cap, uint64_t* out_offsets,
                                      uint64_t* out_bytes, void* stream)
try {
	const ContextLines c = {before, after, out_lines, out_line_flags, out_line_spans, line_cap, out_sel_count, out_group_count, out_hit_count};
	const LinesGather gather = {tail, out_text, text_cap, out_offsets, out_bytes, true, "hipMallocAsync(line spans)"};
	return RunLinesContextImpl("pire_hip_run_lines_context_gather", t, raw, size, delim, flags, want, c, out_line_count, &gather, stream);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_slow_lines_context_select(pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint32_t mode,
                                       uint64_t before, uint64_t after, uint64_t* out_line_count, uint64_t* out_lines, uint8_t* out_line_flags,
                                       uint64_t* out_line_spans, uint64_t line_cap, uint64_t* out_sel_count, uint64_t* out_group_count,
                                       uint64_t* out_hit_count, void* stream)
try {
	const ContextLines c = {before, after, out_lines, out_line_flags, out_line_spans, line_cap, out_sel_count, out_group_count, out_hit_count};
	return SlowLinesContextImpl("pire_hip_slow_lines_context_select", t, raw, size, delim, flags, mode, c, out_line_count, nullptr, stream);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_slow_lines_context_gather(pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint32_t mode,
                                       uint64_t before, uint64_t after, uint64_t* out_line_count, uint64_t* out_lines, uint8_t* out_line_flags,
                                       uint64_t* out_line_spans, uint64_t line_cap, uint64_t* out_sel_count, uint64_t* out_group_count,
                                       uint64_t* out_hit_count, uint32_t tail, void* out_text, uint64_t text_cap, uint64_t* out_offsets,
                                       uint64_t* out_bytes, void* stream)
try {
	const ContextLines c = {before, after, out_lines, out_line_flags, out_line_spans, line_cap, out_sel_count, out_group_count, out_hit_count};
	const LinesGather gather = {tail, out_text, text_cap, out_offsets, out_bytes, true, "hipMallocAsync(line spans)"};
	return SlowLinesContextImpl("pire_hip_slow_lines_context_gather", t, raw, size, delim, flags, mode, c, out_line_count, &gather, stream);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- the bytes of many files in, the matching lines by file out (split.hip, files.hip) ---------------------------------------
// The frame around scan + hit list + pire_hip_files: the hit list of the scan lives in scratch, whole -- a file's count does not
// depend on hit_cap --, the pass copies what the caller has room for.  The frame takes no table: the scan is the entry point's
// own call (Scanner: with `want` staged in; SlowScanner: with `mode`).
namespace {

struct FilesLines {
	const uint64_t* fileBytes;
	uint64_t files;
	uint32_t fileMode;
	uint64_t *outHits, *outHitSpans, *outHitFile, *outHitLine;
	uint64_t hitCap;
	uint64_t *outHitCount, *outFileLines, *outFileFirst, *outFiles;
	uint64_t fileCap;
	uint64_t *outFileCount, *outStraddles;
};

// scan(f, dWant, dHits, dHitCount): the hit list of the lines f.Text() / f.Offsets() / f.n into dHits[f.n], their number into *dHitCount
int FilesLinesImpl(const char* who, const char* refused, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, const uint64_t* want,
                   uint32_t wantWords, const FilesLines& c, uint64_t* out_line_count, void* streamPtr,
                   const std::function<int(const LinesFrame&, const uint64_t*, uint64_t*, uint64_t*)>& scan)
{
	if (refused)
		return GatherRefuse(who, refused);
	if (!c.outHitCount)
		return GatherRefuse(who, "null out_hit_count");
	if (c.hitCap && !c.outHits)
		return GatherRefuse(who, "hit_cap > 0 with null out_hits");
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	if (c.outHitSpans && !c.outHits)
		return GatherRefuse(who, "out_hit_spans without out_hits");
	const FilesOut o = {c.outFiles, c.fileCap, c.outFileCount};
	if (int rc = FilesArgsInvalid(who, c.fileBytes != nullptr, "file_bytes", c.files, c.fileMode, o))
		return rc;
	if (!c.outStraddles)
		return GatherRefuse(who, "null out_straddles");
	if (c.files == 0 && size)
		return GatherRefuse(who, "files == 0 with size > 0");
	LinesFrame f(who, raw, size, delim, flags, nullptr, streamPtr);
	if (!f.onDevice)
		if (int rc = FilesBoundsInvalid(who, "file_bytes", c.fileBytes, c.files, size, "size"))
			return rc;
	const uint64_t files = c.files;
	if (f.HostEdge(out_line_count)) {
		// no bytes: no line, no hit, every file empty
		*c.outHitCount = 0;
		*c.outStraddles = 0;
		for (uint64_t k = 0; k <= files; ++k) {
			if (c.outFileLines)
				c.outFileLines[k] = 0;
			if (c.outFileFirst)
				c.outFileFirst[k] = 0;
		}
		*c.outFileCount = c.fileMode & PIRE_HIP_FILES_WITHOUT ? files : 0;
		for (uint64_t k = 0; k < std::min(*c.outFileCount, c.fileCap); ++k)
			c.outFiles[k] = k;
		return PIRE_HIP_OK;
	}
	const uint64_t *dWant = nullptr, *dFileBytes = nullptr;
	uint64_t *dHitFile = nullptr, *dHitLine = nullptr, *dFileLines = nullptr, *dFileFirst = nullptr, *dFiles = nullptr, *dFileCount = nullptr,
	         *dStraddles = nullptr;
	if (int rc = f.Open())
		return rc;
	if (want)
		if (int rc = f.io.In(want, size_t(wantWords), &dWant))
			return rc;
	if (files)
		if (int rc = f.io.In(c.fileBytes, size_t(files) + 1, &dFileBytes))
			return rc;
	if (int rc = f.Split(out_line_count, c.outHitCount, 1, c.hitCap, true))
		return rc;
	if (int rc = f.Lists(c.outHits, c.outHitSpans))
		return rc;
	const uint64_t listCap = std::min(c.fileCap, files);   // `files` files: no list is staged longer
	if (c.outHitFile && f.cap)
		if (int rc = f.io.Result(c.outHitFile, size_t(f.cap), 0, &dHitFile))
			return rc;
	if (c.outHitLine && f.cap)
		if (int rc = f.io.Result(c.outHitLine, size_t(f.cap), 0, &dHitLine))
			return rc;
	if (c.outFileLines)
		if (int rc = f.io.Result(c.outFileLines, size_t(files) + 1, size_t(files) + 1, &dFileLines))
			return rc;
	if (c.outFileFirst)
		if (int rc = f.io.Result(c.outFileFirst, size_t(files) + 1, size_t(files) + 1, &dFileFirst))
			return rc;
	if (c.outFiles && listCap)
		if (int rc = f.io.Result(c.outFiles, size_t(listCap), 0, &dFiles))
			return rc;
	if (int rc = f.io.Result(c.outFileCount, 1, 1, &dFileCount))
		return rc;
	if (int rc = f.io.Result(c.outStraddles, 1, 1, &dStraddles))
		return rc;
	StreamScratch hitList(f.stream), ownLines(f.stream);   // (live until the pass behind the scan is enqueued)
	if (!dFileLines) {
		if (int rc = ownLines.Alloc((size_t(files) + 1) * 8, "hipMallocAsync(file lines)"))
			return rc;
		dFileLines = ownLines.as<uint64_t>();
	}
	// the scan's hit list: 8 bytes a line at most
	if (int rc = hitList.Alloc((size_t(f.n) + 1) * 8, "hipMallocAsync(files hits)"))
		return rc;
	uint64_t* dScanHits = hitList.as<uint64_t>();
	if (f.n == 0) {
		if (int rc = f.ZeroCounts("hipMemsetAsync(hit count)"))
			return rc;
	} else {
		if (int rc = scan(f, dWant, dScanHits, f.dCounts))
			return rc;
	}
	if (int rc = LaunchFileLines(f.LineOffsets(), f.n, dFileBytes, files, f.dRaw, size, delim, dFileLines, dStraddles, f.stream))
		return rc;
	if (int rc = LaunchFiles(dScanHits, f.dCounts, f.n, dFileLines, files, c.fileMode, dFileFirst, f.dHits, dHitFile, dHitLine, f.dHits ? f.cap : 0,
	                         dFiles, listCap, dFileCount, f.stream))
		return rc;
	if (f.dSpans)   // (the whole line)
		if (int rc = LaunchHitSpans(f.dHits, f.dCounts, 1, f.cap, f.cap, f.LineOffsets(), f.dSpans, f.stream, "split spans launch"))
			return rc;
	if (int rc = f.Close("hipMemcpy(hits)"))
		return rc;
	if (f.onDevice)
		return PIRE_HIP_OK;
	if (int rc = HitsBack(1, c.outHitCount, f.cap, f.cap, dHitFile, c.outHitFile, 8, "hipMemcpy(hit files)"))
		return rc;
	if (int rc = HitsBack(1, c.outHitCount, f.cap, f.cap, dHitLine, c.outHitLine, 8, "hipMemcpy(hit files)"))
		return rc;
	return HitsBack(1, c.outFileCount, listCap, listCap, dFiles, c.outFiles, 8, "hipMemcpy(files)");
}

}  // namespace

int pire_hip_run_lines_files_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, const uint64_t* want,
                                    const uint64_t* file_bytes, uint64_t files, uint32_t file_mode, uint64_t* out_line_count, uint64_t* out_hits,
                                    uint64_t* out_hit_spans, uint64_t* out_hit_file, uint64_t* out_hit_line, uint64_t hit_cap,
                                    uint64_t* out_hit_count, uint64_t* out_file_lines, uint64_t* out_file_first, uint64_t* out_files,
                                    uint64_t file_cap, uint64_t* out_file_count, uint64_t* out_straddles, void* stream)
try {
	const FilesLines c = {file_bytes, files, file_mode, out_hits, out_hit_spans, out_hit_file, out_hit_line, hit_cap, out_hit_count,
	                      out_file_lines, out_file_first, out_files, file_cap, out_file_count, out_straddles};
	return FilesLinesImpl("pire_hip_run_lines_files_select", t ? nullptr : "null table", raw, size, delim, flags, want,
	                      t ? pire_hip_table_mask_words(t) : 0, c, out_line_count, stream,
	                      [&](const LinesFrame& f, const uint64_t* dWant, uint64_t* dHits, uint64_t* dHitCount) {
		                      return pire_hip_run_select(t, f.Text(), f.Offsets(), f.n, f.RunFlags(), nullptr, nullptr, nullptr, nullptr, dWant,
		                                                 nullptr, dHits, nullptr, f.n, dHitCount, f.stream);
	                      });
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_slow_lines_files_select(pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint32_t mode,
                                     const uint64_t* file_bytes, uint64_t files, uint32_t file_mode, uint64_t* out_line_count, uint64_t* out_hits,
                                     uint64_t* out_hit_spans, uint64_t* out_hit_file, uint64_t* out_hit_line, uint64_t hit_cap,
                                     uint64_t* out_hit_count, uint64_t* out_file_lines, uint64_t* out_file_first, uint64_t* out_files,
                                     uint64_t file_cap, uint64_t* out_file_count, uint64_t* out_straddles, void* stream)
try {
	const FilesLines c = {file_bytes, files, file_mode, out_hits, out_hit_spans, out_hit_file, out_hit_line, hit_cap, out_hit_count,
	                      out_file_lines, out_file_first, out_files, file_cap, out_file_count, out_straddles};
	return FilesLinesImpl("pire_hip_slow_lines_files_select", !t ? "null table" : mode > PIRE_HIP_FINAL_SELECT_ZERO ? "unknown mode" : nullptr,
	                      raw, size, delim, flags, nullptr, 0, c, out_line_count, stream,
	                      [&](const LinesFrame& f, const uint64_t*, uint64_t* dHits, uint64_t* dHitCount) {
		                      return pire_hip_slow_run_select(t, f.Text(), f.Offsets(), f.n, f.RunFlags(), mode, nullptr, nullptr, nullptr, dHits,
		                                                      f.n, dHitCount, f.stream);
	                      });
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- raw bytes in, the lines a boolean function of several scans selects out (split.hip, fields.hip, combine.hip) ----------
// The frame around k scans + their hit lists + pire_hip_combine: one split, one cut per distinct column, every term's list
// in scratch (8 bytes a line a term at most), the combined list in the place the hit list has in the forms above -- hits,
// spans, the gather through the spans.  Every term scans with its own table, `want` / mode and run flags.
namespace {

struct CombineLines {
	uint64_t truth;
	uint64_t* outHits;
	uint64_t* outSpans;
	uint8_t* outMembers;
	uint64_t hitCap;
	uint64_t *outHitCount, *outTermCounts;
};

int CombineLinesImpl(const char* who, const pire_hip_line_term* terms, uint32_t kTerms, const CombineLines& c, const void* raw, uint64_t size,
                     uint32_t delim, uint32_t flags, uint64_t* out_line_count, const LinesGather* gather, void* streamPtr)
{
	if (!terms)
		return GatherRefuse(who, "null terms");
	if (kTerms == 0 || kTerms > PIRE_HIP_COMBINE_MAX_LISTS)
		return GatherRefuse(who, kTerms ? "more than 6 terms" : "k_terms == 0");
	if (flags & ~uint32_t(PIRE_HIP_RUN_ON_DEVICE))
		return GatherRefuse(who, "flags other than PIRE_HIP_RUN_ON_DEVICE (BEGIN / END are each term's own)");
	for (uint32_t j = 0; j < kTerms; ++j) {
		const pire_hip_line_term& t = terms[j];
		const std::string term = "term " + std::to_string(j) + ": ";
		if (!t.table == !t.slow_table)
			return GatherRefuse(who, (term + (t.table ? "both table and slow_table" : "neither table nor slow_table")).c_str());
		if (t.slow_table && t.mode > PIRE_HIP_FINAL_SELECT_ZERO)
			return GatherRefuse(who, (term + "unknown mode").c_str());
		if (t.run_flags & ~uint32_t(PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END | PIRE_HIP_RUN_GENERIC))
			return GatherRefuse(who, (term + "unknown bits in run_flags").c_str());
		if (t.column != PIRE_HIP_TERM_LINE) {
			if (int rc = FieldArgsInvalid(who, t.sep, t.field_mode))
				return rc;
			if (t.sep == delim)
				return GatherRefuse(who, (term + "sep == delim").c_str());
		}
	}
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	// (the gather form keeps the hit list to itself where the caller has no array for it)
	const CombineOut o = {c.outHits, c.outMembers, c.hitCap, c.outHitCount};
	if (int rc = CombineOutputsInvalid(who, 0, o, gather != nullptr))
		return rc;
	if (c.outSpans && !c.outHits)
		return GatherRefuse(who, "out_hit_spans without out_hits");
	if (gather) {
		if (int rc = GatherOutputsInvalid(who, "hit_cap", c.hitCap, gather->tail, gather->outText, gather->textCap, gather->outOffsets,
		                                  gather->outBytes))
			return rc;
		if (int rc = GatherOverlaps(who, raw, size, gather->outText, gather->textCap))
			return rc;
	}
	LinesFrame f(who, raw, size, delim, flags, gather, streamPtr);
	if (f.HostEdge(out_line_count)) {
		*c.outHitCount = 0;
		for (uint32_t j = 0; j < kTerms && c.outTermCounts; ++j)
			c.outTermCounts[j] = 0;
		return PIRE_HIP_OK;
	}
	const uint64_t* dWant[PIRE_HIP_COMBINE_MAX_LISTS] = {};
	uint8_t* dMembers = nullptr;
	uint64_t* dTermCounts = nullptr;
	if (int rc = f.Open())
		return rc;
	for (uint32_t j = 0; j < kTerms; ++j)
		if (terms[j].table && terms[j].want)
			if (int rc = f.io.In(terms[j].want, size_t(pire_hip_table_mask_words(terms[j].table)), &dWant[j]))
				return rc;
	if (int rc = f.Split(out_line_count, c.outHitCount, 1, c.hitCap, true))
		return rc;
	if (int rc = f.Lists(c.outHits, c.outSpans))
		return rc;
	if (c.outHits && c.outMembers && f.cap)
		if (int rc = f.io.Result(c.outMembers, size_t(f.cap), 0, &dMembers))
			return rc;
	if (c.outTermCounts)
		if (int rc = f.io.Result(c.outTermCounts, size_t(kTerms), size_t(kTerms), &dTermCounts))
			return rc;
	StreamScratch termLists(f.stream);   // (lives until the pass behind the scans is enqueued)
	std::vector<std::unique_ptr<StreamScratch>> cuts;   // one per distinct column, alive until the scans are enqueued
	if (f.n == 0) {
		if (int rc = f.ZeroCounts("hipMemsetAsync(hit count)"))
			return rc;
		const hipError_t e = dTermCounts ? hipMemsetAsync(dTermCounts, 0, size_t(kTerms) * 8, f.stream) : hipSuccess;
		if (e != hipSuccess)
			return HipFail(e, "hipMemsetAsync(term counts)");
	} else {
		// the terms' hit lists: 8 bytes a line a term at most, and their counts where the caller has no place for them
		if (int rc = termLists.Alloc((size_t(f.n) + 1) * 8 * kTerms, "hipMallocAsync(term hits)"))
			return rc;
		uint64_t* base = termLists.as<uint64_t>();
		if (!dTermCounts)
			dTermCounts = base + size_t(f.n) * kTerms;
		const void* text[PIRE_HIP_COMBINE_MAX_LISTS];
		const uint64_t* offsets[PIRE_HIP_COMBINE_MAX_LISTS];
		for (uint32_t j = 0; j < kTerms; ++j) {
			const pire_hip_line_term& t = terms[j];
			if (t.column == PIRE_HIP_TERM_LINE) {
				text[j] = f.lines.text.get(), offsets[j] = f.LineOffsets();
				continue;
			}
			uint32_t same = j;   // an earlier term with the same cut
			for (uint32_t i = 0; i < j && same == j; ++i)
				if (terms[i].column == t.column && terms[i].sep == t.sep && terms[i].field_mode == t.field_mode)
					same = i;
			if (same == j) {
				cuts.push_back(std::make_unique<StreamScratch>(f.stream));
				const LinesField column = {t.sep, t.column, t.field_mode};
				if (int rc = f.Cut(column, *cuts.back()))
					return rc;
				text[j] = f.cutText, offsets[j] = f.cutOffsets;
			} else {
				text[j] = text[same], offsets[j] = offsets[same];
			}
		}
		f.cutText = nullptr, f.cutOffsets = nullptr;   // (the frame itself goes on with the whole lines)
		CombineLists in = {};
		in.k = kTerms;
		for (uint32_t j = 0; j < kTerms; ++j) {
			const pire_hip_line_term& t = terms[j];
			uint64_t* list = base + size_t(f.n) * j;
			const uint32_t runFlags = t.run_flags | PIRE_HIP_RUN_ON_DEVICE;
			const int rc = t.table ? pire_hip_run_select(t.table, text[j], offsets[j], f.n, runFlags, nullptr, nullptr, nullptr, nullptr, dWant[j],
			                                             nullptr, list, nullptr, f.n, dTermCounts + j, f.stream)
			                       : pire_hip_slow_run_select(t.slow_table, text[j], offsets[j], f.n, runFlags, t.mode, nullptr, nullptr, nullptr,
			                                                  list, f.n, dTermCounts + j, f.stream);
			if (rc)
				return rc;
			in.lists[j] = list, in.counts[j] = dTermCounts + j, in.caps[j] = f.n;
		}
		if (int rc = LaunchCombine(in, f.n, c.truth, f.dHits, dMembers, f.dHits ? f.cap : 0, f.dCounts, f.stream))
			return rc;
		if (f.dSpans)   // (the whole line, whatever part of it was scanned)
			if (int rc = LaunchHitSpans(f.dHits, f.dCounts, 1, f.cap, f.cap, f.LineOffsets(), f.dSpans, f.stream, "split spans launch"))
				return rc;
	}
	if (int rc = f.Close("hipMemcpy(combined hits)"))
		return rc;
	return f.onDevice ? PIRE_HIP_OK : HitsBack(1, c.outHitCount, f.cap, f.cap, dMembers, c.outMembers, 1, "hipMemcpy(combined hits)");
}

}  // namespace

int pire_hip_lines_combine_select(const pire_hip_line_term* terms, uint32_t k_terms, uint64_t truth, const void* raw, uint64_t size,
                                  uint32_t delim, uint32_t flags, uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans,
                                  uint8_t* out_hit_members, uint64_t hit_cap, uint64_t* out_hit_count, uint64_t* out_term_counts, void* stream)
try {
	const CombineLines c = {truth, out_hits, out_hit_spans, out_hit_members, hit_cap, out_hit_count, out_term_counts};
	return CombineLinesImpl("pire_hip_lines_combine_select", terms, k_terms, c, raw, size, delim, flags, out_line_count, nullptr, stream);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_lines_combine_gather(const pire_hip_line_term* terms, uint32_t k_terms, uint64_t truth, const void* raw, uint64_t size,
                                  uint32_t delim, uint32_t flags, uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans,
                                  uint8_t* out_hit_members, uint64_t hit_cap, uint64_t* out_hit_count, uint64_t* out_term_counts, uint32_t tail,
                                  void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* stream)
try {
	const CombineLines c = {truth, out_hits, out_hit_spans, out_hit_members, hit_cap, out_hit_count, out_term_counts};
	const LinesGather gather = {tail, out_text, text_cap, out_offsets, out_bytes, true, "hipMallocAsync(hit spans)"};
	return CombineLinesImpl("pire_hip_lines_combine_gather", terms, k_terms, c, raw, size, delim, flags, out_line_count, &gather, stream);
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// The scan parameters of the prefix and the suffix searches (the caller holds the table: TableUse), for pire_hip_prefix /
// pire_hip_suffix and for the calls that run both (pire_hip_affix_run_select)
static int PrefixParams(pire_hip_table* t, ScanParams* p, bool throughBegin)
{
	if (int rc = FillParams(t, p, throughBegin ? PIRE_HIP_RUN_BEGIN : 0, /*wantDist=*/true))   // startPerm = Initialize [+ BeginMark]
		return rc;
	p->actDist = p->distFlaggedPerm;
	return PIRE_HIP_OK;
}
static int SuffixParams(pire_hip_table* t, ScanParams* p, bool throughEnd)
{
	if (int rc = FillParams(t, p, 0))
		return rc;
	if (throughEnd) {   // Initialize, then Step(EndMark): run.h:319-320 / 349-350
		const HostTable& h = t->host;
		p->startPerm = p->hostPermOfOrig[h.next[size_t(h.initial) * h.letters + h.cls[kEndMark]]];
	}
	return PIRE_HIP_OK;
}

int pire_hip_prefix(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, int longest,
                    int through_begin, int through_end, uint32_t flags, int64_t* out_len, void* streamPtr)
try {
	if (!t || (n && (!offsets || !out_len))) {
		SetError("null argument");
		return PIRE_HIP_EINVAL;
	}
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	if (n)
		if (int rc = SelfTestPrefix(t, false, through_begin, through_end, stream))   // first use on this device (selftest.h)
			return rc;
	ScanParams p;
	TableUse use(t, (flags & PIRE_HIP_RUN_ON_DEVICE) != 0);
	if (int rc = PrefixParams(t, &p, through_begin != 0))
		return rc;
	p.n = n;
	if (n == 0)
		return PIRE_HIP_OK;
	BatchIO io(stream, (flags & PIRE_HIP_RUN_ON_DEVICE) != 0);
	long long* dOut = nullptr;
	if (int rc = io.Text(text, offsets, n, 0, 0, &p.text, &p.offsets))
		return rc;
	if (int rc = io.Result(reinterpret_cast<long long*>(out_len), size_t(n), size_t(n), &dOut))
		return rc;
	if (int rc = io.Ready())
		return rc;
	if (int rc = LaunchPrefix(p, longest != 0, through_end != 0, dOut, stream, (flags & PIRE_HIP_RUN_GENERIC) ? nullptr : NextWorkSlot(t, p)))
		return rc;
	return io.Finish();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// Pire::Run(scanner1, scanner2, state1, state2, begin, end) (run.h:229-241) / Runner over ScannerPair (pair.h:33-94).
static int RunPairImpl(pire_hip_table* t1, pire_hip_table* t2, const void* text, const uint64_t* offsets, uint64_t n,
                       uint64_t len, uint64_t stride, uint32_t flags, uint32_t* outIdx1, uint32_t* outIdx2,
                       uint8_t* outFinal, void* streamPtr)
{
	if (!t1 || !t2) {
		SetError("null table");
		return PIRE_HIP_EINVAL;
	}
	if (!(flags & PIRE_HIP_RUN_ON_DEVICE)) {
		SetError("pire_hip_run_pair takes device pointers (PIRE_HIP_RUN_ON_DEVICE): stage the text once, scan it with both");
		return PIRE_HIP_EINVAL;
	}
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	flags &= PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END | PIRE_HIP_RUN_ON_DEVICE | PIRE_HIP_RUN_GENERIC;
	ScanParams a, b;
	TableUse use1, use2;   // in address order: two calls with the tables swapped must not wait for each other
	use1.Acquire(t1 < t2 ? t1 : t2, true);
	if (t1 != t2)
		use2.Acquire(t1 < t2 ? t2 : t1, true);
	if (int rc = FillParams(t1, &a, flags))
		return rc;
	if (int rc = FillParams(t2, &b, flags))
		return rc;
	if (n == 0)
		return PIRE_HIP_OK;
	a.n = b.n = n;
	a.len = b.len = len;
	a.stride = b.stride = stride;
	a.text = b.text = static_cast<const uint8_t*>(text);
	a.offsets = b.offsets = offsets;
	a.outIdx = outIdx1;
	a.outFinal = outFinal;
	uint64_t fused = 0;
	if (!offsets && !(flags & PIRE_HIP_RUN_GENERIC) && PairTiledEligible(a, b)) {
		if (int rc = LaunchPairTiled(a, b, outIdx2, stream))
			return rc;
		fused = n & ~uint64_t(63);
		if (fused == n)
			return PIRE_HIP_OK;
	}
	// what is left (everything, when the batch is not made of fixed-length records): two ordinary passes, Final = either
	const uint64_t rest = n - fused;
	StreamScratch fin2(stream);
	if (outFinal)
		if (int rc = fin2.Alloc(size_t(rest), "hipMallocAsync(pair finals)"))
			return rc;
	auto shift = [&](ScanParams& p, uint32_t* idx, uint8_t* fin) {
		p.n = rest;
		if (!offsets)
			p.text += fused * stride;
		else
			p.offsets += fused;
		p.outIdx = idx ? idx + fused : nullptr;
		p.outFinal = fin;
	};
	shift(a, outIdx1, outFinal ? outFinal + fused : nullptr);
	shift(b, outIdx2, fin2.as<uint8_t>());
	if (int rc = Dispatch(a, stream, NextWorkSlot(t1, a), offsets ? ~0ull : 0))
		return rc;
	if (int rc = Dispatch(b, stream, NextWorkSlot(t2, b), offsets ? ~0ull : 0))
		return rc;
	return outFinal ? LaunchOrFinal(outFinal + fused, fin2.as<const uint8_t>(), rest, stream) : PIRE_HIP_OK;
}

int pire_hip_run_pair(pire_hip_table* t1, pire_hip_table* t2, const void* text, const uint64_t* offsets, uint64_t n,
                      uint32_t flags, uint32_t* out_state_idx1, uint32_t* out_state_idx2, uint8_t* out_final, void* stream)
try {
	if (n && !offsets) {
		SetError("null offsets");
		return PIRE_HIP_EINVAL;
	}
	return RunPairImpl(t1, t2, text, offsets, n, 0, 0, flags, out_state_idx1, out_state_idx2, out_final, stream);
} catch (...) {
	return pirehip::HandleException();
}

int pire_hip_run_pair_strided(pire_hip_table* t1, pire_hip_table* t2, const void* text, uint64_t n, uint64_t len,
                              uint64_t stride, uint32_t flags, uint32_t* out_state_idx1, uint32_t* out_state_idx2,
                              uint8_t* out_final, void* stream)
try {
	if (stride < len) {
		SetError("stride smaller than len");
		return PIRE_HIP_EINVAL;
	}
	return RunPairImpl(t1, t2, text, nullptr, n, len, stride, flags, out_state_idx1, out_state_idx2, out_final, stream);
} catch (...) {
	return pirehip::HandleException();
}

int pire_hip_suffix(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, int longest,
                    int through_end, int through_begin, uint32_t flags, int64_t* out_len, void* streamPtr)
try {
	if (!t || (n && (!offsets || !out_len))) {
		SetError("null argument");
		return PIRE_HIP_EINVAL;
	}
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	if (n)
		if (int rc = SelfTestPrefix(t, true, through_end, through_begin, stream))   // first use on this device (selftest.h)
			return rc;
	ScanParams p;
	TableUse use(t, (flags & PIRE_HIP_RUN_ON_DEVICE) != 0);
	if (int rc = SuffixParams(t, &p, through_end != 0))
		return rc;
	p.n = n;
	if (n == 0)
		return PIRE_HIP_OK;
	BatchIO io(stream, (flags & PIRE_HIP_RUN_ON_DEVICE) != 0);
	long long* dOut = nullptr;
	if (int rc = io.Text(text, offsets, n, 0, 0, &p.text, &p.offsets))
		return rc;
	if (int rc = io.Result(reinterpret_cast<long long*>(out_len), size_t(n), size_t(n), &dOut))
		return rc;
	if (int rc = io.Ready())
		return rc;
	if (int rc = LaunchSuffix(p, longest != 0, through_begin != 0, dOut, stream))
		return rc;
	return io.Finish();
} catch (...) {
	return pirehip::HandleException();
}

// ---- the matched heads and tails of a batch (exact.hip, affix.hip) and of the lines of a buffer ------------------------------
namespace {

// The two scans of the affix forms, as the caller of an entry point gave them (either table may be null, not both)
struct AffixScans {
	pire_hip_table* head;
	uint32_t headOpts;
	pire_hip_table* tail;
	uint32_t tailOpts;
};

int AffixScansInvalid(const char* who, const AffixScans& s)
{
	const uint32_t known = PIRE_HIP_AFFIX_LONGEST | PIRE_HIP_AFFIX_THROUGH_BEGIN | PIRE_HIP_AFFIX_THROUGH_END;
	const char* what = !s.head && !s.tail      ? "null head and null tail"
	                   : s.headOpts & ~known   ? "unknown bits in head_opts"
	                   : s.tailOpts & ~known   ? "unknown bits in tail_opts"
	                                           : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

// Both tables held still for one entry point, and their scan parameters.  Prepare (n > 0): each scan's first-use self-test
// (it calls the scan's own entry point: before the tables are held), then the tables in address order -- two calls with the
// tables swapped must not wait for each other (RunPairImpl) --, then the parameters.
struct AffixTables {
	TableUse use1, use2;
	ScanParams ph, pt;
	int Prepare(const AffixScans& s, bool enqueueOnly, hipStream_t stream)
	{
		if (s.head)
			if (int rc = SelfTestPrefix(s.head, false, (s.headOpts & PIRE_HIP_AFFIX_THROUGH_BEGIN) != 0, (s.headOpts & PIRE_HIP_AFFIX_THROUGH_END) != 0,
			                            stream))
				return rc;
		if (s.tail)
			if (int rc = SelfTestPrefix(s.tail, true, (s.tailOpts & PIRE_HIP_AFFIX_THROUGH_END) != 0, (s.tailOpts & PIRE_HIP_AFFIX_THROUGH_BEGIN) != 0,
			                            stream))
				return rc;
		pire_hip_table* first = !s.head ? s.tail : !s.tail ? s.head : std::min(s.head, s.tail);
		pire_hip_table* second = s.head && s.tail && s.head != s.tail ? std::max(s.head, s.tail) : nullptr;
		use1.Acquire(first, enqueueOnly);
		if (second)
			use2.Acquire(second, enqueueOnly);
		if (s.head)
			if (int rc = PrefixParams(s.head, &ph, (s.headOpts & PIRE_HIP_AFFIX_THROUGH_BEGIN) != 0))
				return rc;
		if (s.tail)
			if (int rc = SuffixParams(s.tail, &pt, (s.tailOpts & PIRE_HIP_AFFIX_THROUGH_END) != 0))
				return rc;
		return PIRE_HIP_OK;
	}
};

// The scans and the pass enqueued on `stream`, device pointers only (n > 0).  dHeadLen / dTailLen: nullable -- what the caller
// has no array for lives in stream-ordered scratch.  shift: as LaunchAffixSelect's.
int AffixEnqueue(const AffixScans& s, AffixTables& tabs, const void* dText, const uint64_t* dOffsets, uint64_t n, uint32_t flags,
                 int64_t* dHeadLen, int64_t* dTailLen, uint32_t part, uint64_t shift, uint64_t* dHits, uint64_t* dSpans, uint64_t cap,
                 uint64_t* dCount, hipStream_t stream)
{
	StreamScratch ownHead(stream), ownTail(stream);
	long long* headLen = reinterpret_cast<long long*>(dHeadLen);
	long long* tailLen = reinterpret_cast<long long*>(dTailLen);
	if (s.head && !headLen) {
		if (int rc = ownHead.Alloc(size_t(n) * 8, "hipMallocAsync(head lengths)"))
			return rc;
		headLen = ownHead.as<long long>();
	}
	if (s.tail && !tailLen) {
		if (int rc = ownTail.Alloc(size_t(n) * 8, "hipMallocAsync(tail lengths)"))
			return rc;
		tailLen = ownTail.as<long long>();
	}
	if (s.head) {
		ScanParams& p = tabs.ph;
		p.n = n;
		p.text = static_cast<const uint8_t*>(dText);
		p.offsets = dOffsets;
		if (int rc = LaunchPrefix(p, (s.headOpts & PIRE_HIP_AFFIX_LONGEST) != 0, (s.headOpts & PIRE_HIP_AFFIX_THROUGH_END) != 0, headLen, stream,
		                          (flags & PIRE_HIP_RUN_GENERIC) ? nullptr : NextWorkSlot(s.head, p)))
			return rc;
	}
	if (s.tail) {
		ScanParams& p = tabs.pt;
		p.n = n;
		p.text = static_cast<const uint8_t*>(dText);
		p.offsets = dOffsets;
		if (int rc = LaunchSuffix(p, (s.tailOpts & PIRE_HIP_AFFIX_LONGEST) != 0, (s.tailOpts & PIRE_HIP_AFFIX_THROUGH_BEGIN) != 0, tailLen, stream))
			return rc;
	}
	return LaunchAffixSelect(dOffsets, n, part, s.head ? headLen : nullptr, s.tail ? tailLen : nullptr, shift, dHits, dSpans, cap, dCount, stream);
}

}  // namespace

int pire_hip_affix_run_select(pire_hip_table* head, uint32_t head_opts, pire_hip_table* tail, uint32_t tail_opts, const void* text,
                              const uint64_t* offsets, uint64_t n, uint32_t part, uint32_t flags, int64_t* out_head_len,
                              int64_t* out_tail_len, uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap, uint64_t* out_hit_count,
                              void* streamPtr)
try {
	const char* who = "pire_hip_affix_run_select";
	const AffixScans scans = {head, head_opts, tail, tail_opts};
	if (int rc = AffixScansInvalid(who, scans))
		return rc;
	const AffixSelectOut o = {part, out_hits, out_spans, hit_cap, out_hit_count};
	if (int rc = AffixSelectArgsInvalid(who, n, offsets != nullptr, head != nullptr, tail != nullptr, o))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	AffixSelectStage pass(o, onDevice);
	if (n == 0)
		return pass.Empty(stream);
	if (!onDevice) {   // what the scans refuse of a host batch, before their self-tests touch a device
		uint64_t textBytes = 0;
		if (int rc = CheckHostBatch(text, offsets, n, 0, 0, &textBytes))
			return rc;
	}
	AffixTables tabs;
	if (int rc = tabs.Prepare(scans, onDevice, stream))
		return rc;
	// host pointers: the text staged once, both scans and the pass on the staged copy, then everything back
	BatchIO io(stream, onDevice);
	const uint8_t* dText = nullptr;
	const uint64_t* dOffsets = nullptr;
	int64_t *dHeadLen = nullptr, *dTailLen = nullptr;
	if (int rc = io.Text(text, offsets, n, 0, 0, &dText, &dOffsets))
		return rc;
	if (head && out_head_len)
		if (int rc = io.Result(out_head_len, size_t(n), size_t(n), &dHeadLen))
			return rc;
	if (tail && out_tail_len)
		if (int rc = io.Result(out_tail_len, size_t(n), size_t(n), &dTailLen))
			return rc;
	if (int rc = pass.Results(io, n))
		return rc;
	if (int rc = io.Ready())
		return rc;
	if (int rc = AffixEnqueue(scans, tabs, dText, dOffsets, n, flags, dHeadLen, dTailLen, part, 0, pass.dHits, pass.dSpans, pass.list.cap, pass.list.dCount,
	                          stream))
		return rc;
	if (int rc = io.Finish())
		return rc;
	return pass.Back();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// The frame around the two searches: the scans on the lines, the pass with shift = 1 (string i of the split buffer lies i bytes
// further into raw), the gather from raw through its spans.
int pire_hip_affix_lines_gather(pire_hip_table* head, uint32_t head_opts, pire_hip_table* tail, uint32_t tail_opts, const void* raw,
                                uint64_t size, uint32_t delim, uint32_t part, uint32_t flags, uint32_t tail_byte, uint64_t* out_line_count,
                                uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap, uint64_t* out_hit_count, void* out_text,
                                uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* streamPtr)
try {
	const char* who = "pire_hip_affix_lines_gather";
	const AffixScans scans = {head, head_opts, tail, tail_opts};
	if (int rc = AffixScansInvalid(who, scans))
		return rc;
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	// no gather output at all: spans only.  (The gather form keeps the span list to itself where the caller has no array for it.)
	const bool gathers = out_text || text_cap || out_offsets || out_bytes;
	const AffixSelectOut o = {part, out_hits, out_spans, hit_cap, out_hit_count};
	if (int rc = AffixSelectArgsInvalid(who, 0, true, head != nullptr, tail != nullptr, o, gathers))
		return rc;
	if (gathers) {
		if (int rc = GatherOutputsInvalid(who, "hit_cap", hit_cap, tail_byte, out_text, text_cap, out_offsets, out_bytes))
			return rc;
		if (int rc = GatherOverlaps(who, raw, size, out_text, text_cap))
			return rc;
	}
	const LinesGather gather = {tail_byte, out_text, text_cap, out_offsets, out_bytes, false, "hipMallocAsync(affix spans)"};
	LinesFrame f(who, raw, size, delim, flags, gathers ? &gather : nullptr, streamPtr);
	if (f.HostEdge(out_line_count)) {
		*out_hit_count = 0;
		return PIRE_HIP_OK;
	}
	if (int rc = f.Open())
		return rc;
	if (int rc = f.Split(out_line_count, out_hit_count, 1, hit_cap, true))
		return rc;
	if (int rc = f.Lists(out_hits, out_spans))
		return rc;
	if (f.n == 0) {
		if (int rc = f.ZeroCounts("hipMemsetAsync(hit count)"))
			return rc;
	} else {
		AffixTables tabs;
		if (int rc = tabs.Prepare(scans, f.onDevice, f.stream))
			return rc;
		if (int rc = AffixEnqueue(scans, tabs, f.Text(), f.Offsets(), f.n, f.RunFlags(), nullptr, nullptr, part, 1, f.dHits, f.dSpans, f.cap,
		                          f.dCounts, f.stream))
			return rc;
	}
	return f.Close("hipMemcpy(affix spans)");
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- where the match lies: the leftmost-longest match of every string (search.hip) and of the lines of a buffer --------------
namespace {

int SearchArgsInvalid(const char* who, pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts)
{
	const uint32_t known = PIRE_HIP_SEARCH_SHORTEST | PIRE_HIP_SEARCH_THROUGH_BEGIN | PIRE_HIP_SEARCH_THROUGH_END;
	const char* what = !rev           ? "null rev"
	                   : !fwd         ? "null fwd"
	                   : opts & ~known ? "unknown bits in opts"
	                                   : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

int SearchBatchInvalid(const char* who, const void* text, const uint64_t* offsets, uint64_t n)
{
	const char* what = n && (!text || !offsets) ? "n > 0 with null text or offsets"
	                   : n >= (1ull << 32)      ? "2^32 strings or more in one call"
	                                            : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

// Both tables held still for one entry point (in address order, as AffixTables), and their scan parameters: R's start state is
// LongestSuffix's, F's the two candidates of the forward leg.
struct SearchTables {
	TableUse use1, use2;
	ScanParams pr, pf;
	uint32_t fwdStartBegin = 0;
	int Prepare(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts, bool enqueueOnly)
	{
		use1.Acquire(std::min(rev, fwd), enqueueOnly);
		if (rev != fwd)
			use2.Acquire(std::max(rev, fwd), enqueueOnly);
		if (int rc = SuffixParams(rev, &pr, (opts & PIRE_HIP_SEARCH_THROUGH_END) != 0))
			return rc;
		if (int rc = FillParams(fwd, &pf, 0))   // startPerm = Initialize()
			return rc;
		const HostTable& h = fwd->host;
		fwdStartBegin = pf.hostPermOfOrig[h.next[size_t(h.initial) * h.letters + h.cls[kBeginMark]]];   // + Step(BeginMark), run.h:282-283
		return PIRE_HIP_OK;
	}
	// the search enqueued on `stream`, device pointers only (n > 0)
	int Enqueue(uint32_t opts, const void* dText, const uint64_t* dOffsets, uint64_t n, int64_t* dBegin, int64_t* dEnd, hipStream_t stream)
	{
		pr.n = n;
		pr.text = static_cast<const uint8_t*>(dText);
		pr.offsets = dOffsets;
		return LaunchSearch(pr, pf, fwdStartBegin, opts, reinterpret_cast<long long*>(dBegin), reinterpret_cast<long long*>(dEnd), stream);
	}
};

// The search and the capture pass behind it on `stream`, device pointers only (n > 0).  dBegin / dEnd: nullable -- what the caller
// has no array for lives in stream-ordered scratch.  shift: as LaunchCaptureSelect's.
int SearchEnqueue(SearchTables& tabs, uint32_t opts, const void* dText, const uint64_t* dOffsets, uint64_t n, int64_t* dBegin, int64_t* dEnd,
                  uint64_t shift, uint64_t* dHits, uint64_t* dSpans, uint64_t cap, uint64_t* dCount, hipStream_t stream)
{
	StreamScratch own(stream);
	if (!dBegin || !dEnd) {
		if (int rc = own.Alloc(size_t(n) * 16, "hipMallocAsync(search positions)"))
			return rc;
		if (!dBegin)
			dBegin = own.as<int64_t>();
		if (!dEnd)
			dEnd = own.as<int64_t>() + n;
	}
	if (int rc = tabs.Enqueue(opts, dText, dOffsets, n, dBegin, dEnd, stream))
		return rc;
	return LaunchCaptureSelect(dOffsets, n, false, reinterpret_cast<const long long*>(dBegin), reinterpret_cast<const long long*>(dEnd), nullptr,
	                           shift, dHits, dSpans, cap, dCount, stream);
}

}  // namespace

int pire_hip_search(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts, const void* text, const uint64_t* offsets, uint64_t n,
                    uint32_t flags, int64_t* out_begin, int64_t* out_end, void* streamPtr)
try {
	const char* who = "pire_hip_search";
	if (int rc = SearchArgsInvalid(who, rev, fwd, opts))
		return rc;
	if (int rc = SearchBatchInvalid(who, text, offsets, n))
		return rc;
	if (!out_begin || !out_end) {
		SetError(std::string(who) + ": null out_begin or out_end");
		return PIRE_HIP_EINVAL;
	}
	if (n == 0)
		return PIRE_HIP_OK;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	if (!onDevice) {   // what the scans refuse of a host batch, before a device is touched
		uint64_t textBytes = 0;
		if (int rc = CheckHostBatch(text, offsets, n, 0, 0, &textBytes))
			return rc;
	}
	SearchTables tabs;
	if (int rc = tabs.Prepare(rev, fwd, opts, onDevice))
		return rc;
	BatchIO io(stream, onDevice);
	const uint8_t* dText = nullptr;
	const uint64_t* dOffsets = nullptr;
	int64_t *dBegin = nullptr, *dEnd = nullptr;
	if (int rc = io.Text(text, offsets, n, 0, 0, &dText, &dOffsets))
		return rc;
	if (int rc = io.Result(out_begin, size_t(n), size_t(n), &dBegin))
		return rc;
	if (int rc = io.Result(out_end, size_t(n), size_t(n), &dEnd))
		return rc;
	if (int rc = io.Ready())
		return rc;
	if (int rc = tabs.Enqueue(opts, dText, dOffsets, n, dBegin, dEnd, stream))
		return rc;
	return io.Finish();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_search_run_select(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts, const void* text, const uint64_t* offsets, uint64_t n,
                               uint32_t flags, int64_t* out_begin, int64_t* out_end, uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap,
                               uint64_t* out_hit_count, void* streamPtr)
try {
	const char* who = "pire_hip_search_run_select";
	if (int rc = SearchArgsInvalid(who, rev, fwd, opts))
		return rc;
	if (int rc = SearchBatchInvalid(who, text, offsets, n))
		return rc;
	if (int rc = CaptureSelectOutputsInvalid(who, n, 0, true, out_hits || out_spans, hit_cap, out_hit_count))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	if (n == 0) {   // the pass itself zeroes the count on the stream; host pointers: no device is touched
		if (onDevice)
			return LaunchCaptureSelect(nullptr, 0, false, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, out_hit_count, stream);
		*out_hit_count = 0;
		return PIRE_HIP_OK;
	}
	if (!onDevice) {
		uint64_t textBytes = 0;
		if (int rc = CheckHostBatch(text, offsets, n, 0, 0, &textBytes))
			return rc;
	}
	SearchTables tabs;
	if (int rc = tabs.Prepare(rev, fwd, opts, onDevice))
		return rc;
	// host pointers: the text staged once, the search and the pass on the staged copy, then everything back
	BatchIO io(stream, onDevice);
	const uint8_t* dText = nullptr;
	const uint64_t* dOffsets = nullptr;
	int64_t *dBegin = nullptr, *dEnd = nullptr;
	if (int rc = io.Text(text, offsets, n, 0, 0, &dText, &dOffsets))
		return rc;
	if (out_begin)
		if (int rc = io.Result(out_begin, size_t(n), size_t(n), &dBegin))
			return rc;
	if (out_end)
		if (int rc = io.Result(out_end, size_t(n), size_t(n), &dEnd))
			return rc;
	HitStage list(onDevice, out_hit_count, "hipMemcpy(hits)");
	uint64_t *dHits = nullptr, *dSpans = nullptr;
	int rc;
	if ((rc = list.Count(io, hit_cap, n)) || (rc = list.List(io, out_hits, 1, &dHits)) || (rc = list.List(io, out_spans, 2, &dSpans)) ||
	    (rc = io.Ready()))
		return rc;
	if ((rc = SearchEnqueue(tabs, opts, dText, dOffsets, n, dBegin, dEnd, 0, dHits, dSpans, list.cap, list.dCount, stream)))
		return rc;
	if ((rc = io.Finish()))
		return rc;
	return list.Back();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// The frame around the search: the search on the lines, the pass with shift = 1 (string i of the split buffer lies i bytes
// further into raw), the gather from raw through its spans.
int pire_hip_search_lines_gather(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts, const void* raw, uint64_t size, uint32_t delim,
                                 uint32_t flags, uint32_t tail_byte, uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_spans,
                                 uint64_t hit_cap, uint64_t* out_hit_count, void* out_text, uint64_t text_cap, uint64_t* out_offsets,
                                 uint64_t* out_bytes, void* streamPtr)
try {
	const char* who = "pire_hip_search_lines_gather";
	if (int rc = SearchArgsInvalid(who, rev, fwd, opts))
		return rc;
	flags &= PIRE_HIP_RUN_ON_DEVICE;   // (the marks are the search's own: opts)
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	// no gather output at all: spans only.  (The gather form keeps the span list to itself where the caller has no array for it.)
	const bool gathers = out_text || text_cap || out_offsets || out_bytes;
	if (int rc = CaptureSelectOutputsInvalid(who, 0, 0, true, out_hits || out_spans || gathers, hit_cap, out_hit_count))
		return rc;
	if (gathers) {
		if (int rc = GatherOutputsInvalid(who, "hit_cap", hit_cap, tail_byte, out_text, text_cap, out_offsets, out_bytes))
			return rc;
		if (int rc = GatherOverlaps(who, raw, size, out_text, text_cap))
			return rc;
	}
	const LinesGather gather = {tail_byte, out_text, text_cap, out_offsets, out_bytes, false, "hipMallocAsync(search spans)"};
	LinesFrame f(who, raw, size, delim, flags, gathers ? &gather : nullptr, streamPtr);
	if (f.HostEdge(out_line_count)) {
		*out_hit_count = 0;
		return PIRE_HIP_OK;
	}
	if (int rc = f.Open())
		return rc;
	if (int rc = f.Split(out_line_count, out_hit_count, 1, hit_cap, true))
		return rc;
	if (int rc = f.Lists(out_hits, out_spans))
		return rc;
	if (f.n == 0) {
		if (int rc = f.ZeroCounts("hipMemsetAsync(hit count)"))
			return rc;
	} else {
		SearchTables tabs;
		if (int rc = tabs.Prepare(rev, fwd, opts, f.onDevice))
			return rc;
		if (int rc = SearchEnqueue(tabs, opts, f.Text(), f.Offsets(), f.n, nullptr, nullptr, 1, f.dHits, f.dSpans, f.cap, f.dCounts, f.stream))
			return rc;
	}
	return f.Close("hipMemcpy(search spans)");
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- every match of every string (search_all.hip) and of the lines of a buffer -------------------------------------------------
namespace {

// What the list forms of the search refuse of their outputs before any device is touched (haveList: the matches have somewhere to go)
int SearchAllOutputsInvalid(const char* who, bool haveList, uint64_t matchCap, const void* outMatchCount)
{
	const char* what = !outMatchCount          ? "null out_match_count"
	                   : matchCap && !haveList ? "match_cap > 0 with null out_owners and null out_spans"
	                                           : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

// The list form of the search enqueued on `stream`, device pointers only
int SearchAllEnqueue(SearchTables& tabs, uint32_t opts, const void* dText, uint64_t textBytes, const uint64_t* dOffsets, uint64_t n, uint64_t shift,
                     uint64_t* dRows, uint64_t* dOwners, uint64_t* dSpans, uint64_t cap, uint64_t* dCount, hipStream_t stream)
{
	tabs.pr.n = n;
	tabs.pr.text = static_cast<const uint8_t*>(dText);
	tabs.pr.offsets = dOffsets;
	return LaunchSearchAll(tabs.pr, tabs.pf, tabs.fwdStartBegin, opts, textBytes, shift, dRows, dOwners, dSpans, cap, dCount, stream);
}

}  // namespace

int pire_hip_search_all(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts, const void* text, uint64_t text_bytes, const uint64_t* offsets,
                        uint64_t n, uint32_t flags, uint64_t* out_rows, uint64_t* out_owners, uint64_t* out_spans, uint64_t match_cap,
                        uint64_t* out_match_count, void* streamPtr)
try {
	const char* who = "pire_hip_search_all";
	if (int rc = SearchArgsInvalid(who, rev, fwd, opts))
		return rc;
	if (int rc = SearchBatchInvalid(who, text, offsets, n))
		return rc;
	if (int rc = SearchAllOutputsInvalid(who, out_owners || out_spans, match_cap, out_match_count))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	if (n == 0) {   // device pointers: the count (and rows[0]) zeroed on the stream; host pointers: no device is touched
		if (onDevice) {
			ScanParams none{};
			return LaunchSearchAll(none, none, 0, opts, 0, 0, out_rows, nullptr, nullptr, 0, out_match_count, stream);
		}
		*out_match_count = 0;
		if (out_rows)
			out_rows[0] = 0;
		return PIRE_HIP_OK;
	}
	uint64_t textBytes = text_bytes;
	if (!onDevice) {   // what the scans refuse of a host batch, before a device is touched
		if (int rc = CheckHostBatch(text, offsets, n, 0, 0, &textBytes))
			return rc;
		if (textBytes > text_bytes) {
			SetError(std::string(who) + ": an offset exceeds text_bytes");
			return PIRE_HIP_EINVAL;
		}
	}
	SearchTables tabs;
	if (int rc = tabs.Prepare(rev, fwd, opts, onDevice))
		return rc;
	// host pointers: the text staged once (offsets[n] bytes of it), the passes on the staged copy, then everything back
	BatchIO io(stream, onDevice);
	const uint8_t* dText = nullptr;
	const uint64_t* dOffsets = nullptr;
	uint64_t* dRows = nullptr;
	if (int rc = io.Text(text, offsets, n, 0, 0, &dText, &dOffsets))
		return rc;
	if (out_rows)
		if (int rc = io.Result(out_rows, size_t(n) + 1, size_t(n) + 1, &dRows))
			return rc;
	HitStage list(onDevice, out_match_count, "hipMemcpy(matches)");
	// (HitStage::Count's part, with this pass's bound: matches are not empty and do not overlap, so a host call stages no more
	// entries than the text has bytes)
	list.cap = onDevice ? match_cap : std::min<uint64_t>(match_cap, textBytes);
	uint64_t *dOwners = nullptr, *dSpans = nullptr;
	int rc;
	if ((rc = io.Result(onDevice ? out_match_count : &list.count, 1, 1, &list.dCount)) || (rc = list.List(io, out_owners, 1, &dOwners)) ||
	    (rc = list.List(io, out_spans, 2, &dSpans)) || (rc = io.Ready()))
		return rc;
	if ((rc = SearchAllEnqueue(tabs, opts, dText, textBytes, dOffsets, n, 0, dRows, dOwners, dSpans, list.cap, list.dCount, stream)))
		return rc;
	if ((rc = io.Finish()))
		return rc;
	return list.Back();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// The frame around the list form of the search: the search on the lines with shift = 1 (string i of the split buffer lies i bytes
// further into raw), the gather from raw through its spans.  A line can have many matches: the lists are match_cap long.
int pire_hip_search_all_lines_gather(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts, const void* raw, uint64_t size, uint32_t delim,
                                     uint32_t flags, uint32_t tail_byte, uint64_t* out_line_count, uint64_t* out_owners, uint64_t* out_spans,
                                     uint64_t match_cap, uint64_t* out_match_count, void* out_text, uint64_t text_cap, uint64_t* out_offsets,
                                     uint64_t* out_bytes, void* streamPtr)
try {
	const char* who = "pire_hip_search_all_lines_gather";
	if (int rc = SearchArgsInvalid(who, rev, fwd, opts))
		return rc;
	flags &= PIRE_HIP_RUN_ON_DEVICE;   // (the marks are the search's own: opts)
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	// no gather output at all: spans only.  (The gather form keeps the span list to itself where the caller has no array for it.)
	const bool gathers = out_text || text_cap || out_offsets || out_bytes;
	if (int rc = SearchAllOutputsInvalid(who, out_owners || out_spans || gathers, match_cap, out_match_count))
		return rc;
	if (gathers) {
		if (int rc = GatherOutputsInvalid(who, "match_cap", match_cap, tail_byte, out_text, text_cap, out_offsets, out_bytes))
			return rc;
		if (int rc = GatherOverlaps(who, raw, size, out_text, text_cap))
			return rc;
	}
	const LinesGather gather = {tail_byte, out_text, text_cap, out_offsets, out_bytes, false, "hipMallocAsync(search spans)"};
	LinesFrame f(who, raw, size, delim, flags, gathers ? &gather : nullptr, streamPtr);
	if (f.HostEdge(out_line_count)) {
		*out_match_count = 0;
		return PIRE_HIP_OK;
	}
	if (int rc = f.Open())
		return rc;
	if (int rc = f.Split(out_line_count, out_match_count, 1, match_cap, false))
		return rc;
	if (!f.onDevice)
		f.cap = std::min<uint64_t>(f.cap, size);   // matches are not empty and do not overlap: a host call stages no more
	if (int rc = f.Lists(out_owners, out_spans))
		return rc;
	if (f.n == 0) {
		if (int rc = f.ZeroCounts("hipMemsetAsync(match count)"))
			return rc;
	} else {
		SearchTables tabs;
		if (int rc = tabs.Prepare(rev, fwd, opts, f.onDevice))
			return rc;
		if (int rc = SearchAllEnqueue(tabs, opts, f.Text(), size, f.Offsets(), f.n, 1, nullptr, f.dHits, f.dSpans, f.cap, f.dCounts, f.stream))
			return rc;
	}
	return f.Close("hipMemcpy(search spans)");
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- labelled matches and tokens (lex.hip) and those of the lines of a buffer -------------------------------------------------------
namespace {

// What both lex entry points refuse of their tables and opts before any device is touched
int LexArgsInvalid(const char* who, pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts)
{
	const uint32_t known = PIRE_HIP_LEX_SHORTEST | PIRE_HIP_LEX_THROUGH_BEGIN | PIRE_HIP_LEX_THROUGH_END | PIRE_HIP_LEX_TOKENS;
	const bool tokens = (opts & PIRE_HIP_LEX_TOKENS) != 0;
	const char* what = opts & ~known                                                                        ? "unknown bits in opts"
	                   : !fwd                                                                               ? "null fwd"
	                   : !rev && !tokens                                                                    ? "null rev without PIRE_HIP_LEX_TOKENS"
	                   : fwd->host.scannerType != 1 || (!tokens && rev->host.scannerType != 1)              ? "a SimpleScanner table"
	                                                                                                        : nullptr;
	if (what) {
		SetError(std::string(who) + ": " + what);
		return PIRE_HIP_EINVAL;
	}
	if (fwd->host.regexps > 64) {
		SetError(std::string(who) + ": fwd has " + std::to_string(fwd->host.regexps) + " regexps; more than 64 have no accept masks");
		return PIRE_HIP_EUNSUPPORTED;
	}
	return PIRE_HIP_OK;
}

int LexOutputsInvalid(const char* who, bool haveList, uint64_t matchCap, const void* outMatchCount)
{
	const char* what = !outMatchCount          ? "null out_match_count"
	                   : matchCap && !haveList ? "match_cap > 0 with null out_owners, out_spans and out_masks"
	                                           : nullptr;
	if (!what)
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

// The tables of one lex entry point held still, and their scan parameters (SearchTables'; token mode: fwd alone, rev is ignored)
struct LexTables {
	TableUse use1, use2;
	ScanParams pr{}, pf;
	uint32_t fwdStartBegin = 0;
	bool tokens = false;
	int Prepare(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts, bool enqueueOnly)
	{
		tokens = (opts & PIRE_HIP_LEX_TOKENS) != 0;
		if (tokens) {
			use1.Acquire(fwd, enqueueOnly);
		} else {
			use1.Acquire(std::min(rev, fwd), enqueueOnly);
			if (rev != fwd)
				use2.Acquire(std::max(rev, fwd), enqueueOnly);
			if (int rc = SuffixParams(rev, &pr, (opts & PIRE_HIP_LEX_THROUGH_END) != 0))
				return rc;
		}
		if (int rc = FillParams(fwd, &pf, 0))   // startPerm = Initialize()
			return rc;
		const HostTable& h = fwd->host;
		fwdStartBegin = pf.hostPermOfOrig[h.next[size_t(h.initial) * h.letters + h.cls[kBeginMark]]];   // + Step(BeginMark), run.h:282-283
		return PIRE_HIP_OK;
	}
	// the pass enqueued on `stream`, device pointers only
	int Enqueue(uint32_t opts, const void* dText, uint64_t textBytes, const uint64_t* dOffsets, uint64_t n, uint64_t shift, uint64_t* dRows,
	            uint64_t* dOwners, uint64_t* dSpans, uint64_t* dMasks, uint64_t cap, uint64_t* dCount, uint64_t* dLabels, hipStream_t stream)
	{
		ScanParams& batch = tokens ? pf : pr;
		batch.n = n;
		batch.text = static_cast<const uint8_t*>(dText);
		batch.offsets = dOffsets;
		return LaunchLex(pr, pf, fwdStartBegin, opts, textBytes, shift, dRows, dOwners, dSpans, dMasks, cap, dCount, dLabels, stream);
	}
};

}  // namespace

int pire_hip_lex(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts, const void* text, uint64_t text_bytes, const uint64_t* offsets,
                 uint64_t n, uint32_t flags, uint64_t* out_rows, uint64_t* out_owners, uint64_t* out_spans, uint64_t* out_masks,
                 uint64_t match_cap, uint64_t* out_match_count, uint64_t* out_label_counts, void* streamPtr)
try {
	const char* who = "pire_hip_lex";
	if (int rc = LexArgsInvalid(who, rev, fwd, opts))
		return rc;
	if (int rc = SearchBatchInvalid(who, text, offsets, n))
		return rc;
	if (int rc = LexOutputsInvalid(who, out_owners || out_spans || out_masks, match_cap, out_match_count))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	const size_t labels = size_t(fwd->host.regexps) + 1;
	if (n == 0) {   // device pointers: the counts (and rows[0]) zeroed on the stream; host pointers: no device is touched
		if (onDevice) {
			ScanParams none{};
			none.regexps = fwd->host.regexps;
			return LaunchLex(none, none, 0, opts, 0, 0, out_rows, nullptr, nullptr, nullptr, 0, out_match_count, out_label_counts, stream);
		}
		*out_match_count = 0;
		if (out_rows)
			out_rows[0] = 0;
		if (out_label_counts)
			std::fill(out_label_counts, out_label_counts + labels, uint64_t(0));
		return PIRE_HIP_OK;
	}
	uint64_t textBytes = text_bytes;
	if (!onDevice) {   // what the scans refuse of a host batch, before a device is touched
		if (int rc = CheckHostBatch(text, offsets, n, 0, 0, &textBytes))
			return rc;
		if (textBytes > text_bytes) {
			SetError(std::string(who) + ": an offset exceeds text_bytes");
			return PIRE_HIP_EINVAL;
		}
	}
	LexTables tabs;
	if (int rc = tabs.Prepare(rev, fwd, opts, onDevice))
		return rc;
	// host pointers: the text staged once (offsets[n] bytes of it), the passes on the staged copy, then everything back
	BatchIO io(stream, onDevice);
	const uint8_t* dText = nullptr;
	const uint64_t* dOffsets = nullptr;
	uint64_t *dRows = nullptr, *dLabels = nullptr;
	if (int rc = io.Text(text, offsets, n, 0, 0, &dText, &dOffsets))
		return rc;
	if (out_rows)
		if (int rc = io.Result(out_rows, size_t(n) + 1, size_t(n) + 1, &dRows))
			return rc;
	if (out_label_counts)
		if (int rc = io.Result(out_label_counts, labels, labels, &dLabels))
			return rc;
	HitStage list(onDevice, out_match_count, "hipMemcpy(lex entries)");
	// (entries are not empty and do not overlap, so a host call stages no more of them than the text has bytes)
	list.cap = onDevice ? match_cap : std::min<uint64_t>(match_cap, textBytes);
	uint64_t *dOwners = nullptr, *dSpans = nullptr, *dMasks = nullptr;
	int rc;
	if ((rc = io.Result(onDevice ? out_match_count : &list.count, 1, 1, &list.dCount)) || (rc = list.List(io, out_owners, 1, &dOwners)) ||
	    (rc = list.List(io, out_spans, 2, &dSpans)) || (rc = list.List(io, out_masks, 1, &dMasks)) || (rc = io.Ready()))
		return rc;
	if ((rc = tabs.Enqueue(opts, dText, textBytes, dOffsets, n, 0, dRows, dOwners, dSpans, dMasks, list.cap, list.dCount, dLabels, stream)))
		return rc;
	if ((rc = io.Finish()))
		return rc;
	return list.Back();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// The frame around pire_hip_lex: the pass on the lines with shift = 1 (string i of the split buffer lies i bytes further into
// raw), the gather from raw through its spans.
int pire_hip_lex_lines_gather(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts, const void* raw, uint64_t size, uint32_t delim,
                              uint32_t flags, uint32_t tail_byte, uint64_t* out_line_count, uint64_t* out_owners, uint64_t* out_spans,
                              uint64_t* out_masks, uint64_t match_cap, uint64_t* out_match_count, uint64_t* out_label_counts, void* out_text,
                              uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* streamPtr)
try {
	const char* who = "pire_hip_lex_lines_gather";
	if (int rc = LexArgsInvalid(who, rev, fwd, opts))
		return rc;
	flags &= PIRE_HIP_RUN_ON_DEVICE;   // (the marks are the pass's own: opts)
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	// no gather output at all: spans only.  (The gather form keeps the span list to itself where the caller has no array for it.)
	const bool gathers = out_text || text_cap || out_offsets || out_bytes;
	if (int rc = LexOutputsInvalid(who, out_owners || out_spans || out_masks || gathers, match_cap, out_match_count))
		return rc;
	if (gathers) {
		if (int rc = GatherOutputsInvalid(who, "match_cap", match_cap, tail_byte, out_text, text_cap, out_offsets, out_bytes))
			return rc;
		if (int rc = GatherOverlaps(who, raw, size, out_text, text_cap))
			return rc;
	}
	const size_t labels = size_t(fwd->host.regexps) + 1;
	const LinesGather gather = {tail_byte, out_text, text_cap, out_offsets, out_bytes, false, "hipMallocAsync(lex spans)"};
	LinesFrame f(who, raw, size, delim, flags, gathers ? &gather : nullptr, streamPtr);
	if (f.HostEdge(out_line_count)) {
		*out_match_count = 0;
		if (out_label_counts)
			std::fill(out_label_counts, out_label_counts + labels, uint64_t(0));
		return PIRE_HIP_OK;
	}
	if (int rc = f.Open())
		return rc;
	if (int rc = f.Split(out_line_count, out_match_count, 1, match_cap, false))
		return rc;
	if (!f.onDevice)
		f.cap = std::min<uint64_t>(f.cap, size);   // entries are not empty and do not overlap: a host call stages no more
	if (int rc = f.Lists(out_owners, out_spans))
		return rc;
	uint64_t *dMasks = nullptr, *dLabels = nullptr;
	if (out_masks && f.cap)
		if (int rc = f.io.Result(out_masks, size_t(f.cap), 0, &dMasks))
			return rc;
	if (out_label_counts)
		if (int rc = f.io.Result(out_label_counts, labels, labels, &dLabels))
			return rc;
	if (f.n == 0) {
		if (int rc = f.ZeroCounts("hipMemsetAsync(entry count)"))
			return rc;
		if (dLabels && hipMemsetAsync(dLabels, 0, labels * 8, f.stream) != hipSuccess)
			return HipFail(hipGetLastError(), "hipMemsetAsync(label counts)");
	} else {
		LexTables tabs;
		if (int rc = tabs.Prepare(rev, fwd, opts, f.onDevice))
			return rc;
		if (int rc = tabs.Enqueue(opts, f.Text(), size, f.Offsets(), f.n, 1, nullptr, f.dHits, f.dSpans, dMasks, f.cap, f.dCounts, dLabels, f.stream))
			return rc;
	}
	if (int rc = f.Close("hipMemcpy(lex spans)"))
		return rc;
	return f.onDevice ? PIRE_HIP_OK : HitsBack(1, out_match_count, f.cap, f.cap, dMasks, out_masks, 8, "hipMemcpy(lex masks)");
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// ---- the matches replaced, the rest kept (splice.hip) ------------------------------------------------------------------------
namespace {

// What both splice entry points refuse of the pieces and of their outputs before any device is touched
int SpliceArgsInvalid(const char* who, const void* head, uint32_t headLen, const void* tail, uint32_t tailLen, uint32_t mode, uint32_t known,
                      const void* outText, uint64_t textCap, const void* outBytes)
{
	const char* what = !outBytes                                                        ? "null out_bytes"
	                   : headLen > PIRE_HIP_SPLICE_PIECE_MAX                            ? "head_len > 256"
	                   : tailLen > PIRE_HIP_SPLICE_PIECE_MAX                            ? "tail_len > 256"
	                   : headLen && !head                                               ? "head_len > 0 with null head"
	                   : tailLen && !tail                                               ? "tail_len > 0 with null tail"
	                   : mode & ~known                                                  ? "unknown bits in mode"
	                   : textCap && !outText                                            ? "text_cap > 0 with null out_text"
	                                                                                    : nullptr;
	return what ? GatherRefuse(who, what) : PIRE_HIP_OK;
}

}  // namespace

int pire_hip_splice(const void* raw, uint64_t size, const uint64_t* spans, const uint64_t* span_count, uint64_t span_cap, const void* head,
                    uint32_t head_len, const void* tail, uint32_t tail_len, uint32_t mode, const uint64_t* offsets, uint64_t n, uint32_t flags,
                    void* out_text, uint64_t text_cap, uint64_t* out_pos, uint64_t* out_offsets, uint64_t* out_bytes, void* streamPtr)
try {
	const char* who = "pire_hip_splice";
	if (int rc = SpliceArgsInvalid(who, head, head_len, tail, tail_len, mode, PIRE_HIP_SPLICE_KEEP, out_text, text_cap, out_bytes))
		return rc;
	if (span_cap && !spans)
		return GatherRefuse(who, "span_cap > 0 with null spans");
	if (!offsets != !out_offsets)
		return GatherRefuse(who, "offsets and out_offsets: one without the other");
	if (size && !raw)
		return GatherRefuse(who, "size > 0 with null raw");
	if (span_cap >= (1ull << 32) || n >= (1ull << 32))
		return GatherRefuse(who, "2^32 spans or strings or more in one call");
	if (int rc = GatherOverlaps(who, raw, size, out_text, text_cap))
		return rc;
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	const bool onDevice = (flags & PIRE_HIP_RUN_ON_DEVICE) != 0;
	// host pointers: the host's own look at the list -- k spans, ascending and disjoint inside raw -- and at the offsets; it
	// knows the need before the device does
	uint64_t k = span_cap, total = kSpliceTotalUnknown;
	if (!onDevice) {
		k = std::min(span_count ? *span_count : span_cap, span_cap);
		uint64_t grown = 0, behind = 0;
		for (uint64_t j = 0; j < k; ++j) {
			const uint64_t b = spans[2 * j], e = spans[2 * j + 1];
			if (b < behind || e < b || e > size)
				return GatherRefuse(who, "spans must ascend, must not overlap and must lie inside raw");
			grown += uint64_t(head_len) + tail_len - ((mode & PIRE_HIP_SPLICE_KEEP) ? 0 : e - b);
			behind = e;
		}
		total = size + grown;
		if (offsets) {
			if (int rc = CheckOffsets(offsets, n))
				return rc;
			if (offsets[n] > size)
				return GatherRefuse(who, "an offset exceeds size");
		}
	}
	BatchIO io(stream, onDevice);
	const uint8_t* dRaw = nullptr;
	const uint64_t *dSpans = nullptr, *dOffsets = nullptr;
	if (int rc = io.In(static_cast<const uint8_t*>(raw), size_t(size), &dRaw))
		return rc;
	if (int rc = io.In(spans, size_t(k) * 2, &dSpans))
		return rc;
	if (offsets)
		if (int rc = io.In(offsets, size_t(n) + 1, &dOffsets))
			return rc;
	uint64_t *dBytes = nullptr, *dPos = nullptr, *dOutOffsets = nullptr;
	uint8_t* dOutText = nullptr;
	const uint64_t room = std::min(total, text_cap);
	if (int rc = io.Result(out_bytes, 1, 1, &dBytes))
		return rc;
	if (out_pos && k)
		if (int rc = io.Result(out_pos, size_t(k), size_t(k), &dPos))
			return rc;
	if (out_offsets)
		if (int rc = io.Result(out_offsets, size_t(n) + 1, size_t(n) + 1, &dOutOffsets))
			return rc;
	if (room)
		if (int rc = io.Result(static_cast<uint8_t*>(out_text), size_t(room), size_t(room), &dOutText))
			return rc;
	if (int rc = io.Ready())
		return rc;
	StreamScratch own(stream);   // where the pieces begin, where the caller has no array for that
	if (!dPos && k) {
		if (int rc = own.Alloc(size_t(k) * 8, "hipMallocAsync(splice positions)"))
			return rc;
		dPos = own.as<uint64_t>();
	}
	if (int rc = LaunchSplice(dRaw, size, dSpans, onDevice ? span_count : nullptr, k, head, head_len, tail, tail_len, mode, dOffsets, n, dOutText, room,
	                          dPos, dOutOffsets, dBytes, total, stream))
		return rc;
	return io.Finish();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

// The frame around the search and the splice: the search on the lines with shift = 1 (its spans are ranges of raw), then the
// splice straight over raw through those spans -- the delimiters are kept text.
int pire_hip_search_lines_splice(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts, const void* raw, uint64_t size, uint32_t delim,
                                 uint32_t flags, const void* head, uint32_t head_len, const void* tail, uint32_t tail_len, uint32_t mode,
                                 uint64_t* out_line_count, uint64_t* out_spans, uint64_t* out_pos, uint64_t match_cap, uint64_t* out_match_count,
                                 void* out_text, uint64_t text_cap, uint64_t* out_bytes, void* streamPtr)
try {
	const char* who = "pire_hip_search_lines_splice";
	if (int rc = SearchArgsInvalid(who, rev, fwd, opts))
		return rc;
	flags &= PIRE_HIP_RUN_ON_DEVICE;   // (the marks are the search's own: opts)
	if (int rc = SplitArgsInvalid(who, raw, size, delim, out_line_count, "out_line_count"))
		return rc;
	if (!out_match_count)
		return GatherRefuse(who, "null out_match_count");
	if (int rc = SpliceArgsInvalid(who, head, head_len, tail, tail_len, mode, PIRE_HIP_SPLICE_KEEP | PIRE_HIP_SPLICE_FIRST, out_text, text_cap,
	                               out_bytes))
		return rc;
	if (match_cap >= (1ull << 32))
		return GatherRefuse(who, "2^32 spans or strings or more in one call");
	if (int rc = GatherOverlaps(who, raw, size, out_text, text_cap))
		return rc;
	const bool first = (mode & PIRE_HIP_SPLICE_FIRST) != 0;
	LinesFrame f(who, raw, size, delim, flags, nullptr, streamPtr);
	if (f.HostEdge(out_line_count)) {
		*out_match_count = 0;
		*out_bytes = 0;
		return PIRE_HIP_OK;
	}
	if (int rc = f.Open())
		return rc;
	if (int rc = f.Split(out_line_count, out_match_count, 1, match_cap, first))   // (FIRST: n lines have at most n first matches)
		return rc;
	if (!first && !f.onDevice)
		f.cap = std::min<uint64_t>(f.cap, size);   // matches are not empty and do not overlap: a host call stages no more
	if (int rc = f.Lists(nullptr, out_spans))
		return rc;
	// the spans and the positions in scratch of the library's own where the caller has no array for them
	StreamScratch ownSpans(f.stream), ownPos(f.stream);
	uint64_t *dSpans = f.dSpans, *dPos = nullptr, *dBytes = nullptr;
	uint8_t* dOutText = nullptr;
	const uint64_t room = f.onDevice ? text_cap : std::min(text_cap, size + f.cap * (uint64_t(head_len) + tail_len));
	if (int rc = f.io.Result(out_bytes, 1, 1, &dBytes))
		return rc;
	if (out_pos && f.cap)
		if (int rc = f.io.Result(out_pos, size_t(f.cap), 0, &dPos))
			return rc;
	if (room)
		if (int rc = f.io.Result(static_cast<uint8_t*>(out_text), size_t(room), 0, &dOutText))
			return rc;
	if (!dSpans && f.cap) {
		if (int rc = ownSpans.Alloc(size_t(f.cap) * 16, "hipMallocAsync(search spans)"))
			return rc;
		dSpans = ownSpans.as<uint64_t>();
	}
	if (!dPos && f.cap) {
		if (int rc = ownPos.Alloc(size_t(f.cap) * 8, "hipMallocAsync(splice positions)"))
			return rc;
		dPos = ownPos.as<uint64_t>();
	}
	if (f.n == 0) {
		if (int rc = f.ZeroCounts("hipMemsetAsync(match count)"))
			return rc;
	} else {
		SearchTables tabs;
		if (int rc = tabs.Prepare(rev, fwd, opts, f.onDevice))
			return rc;
		if (first) {
			if (int rc = SearchEnqueue(tabs, opts, f.Text(), f.Offsets(), f.n, nullptr, nullptr, 1, nullptr, dSpans, f.cap, f.dCounts, f.stream))
				return rc;
		} else if (int rc = SearchAllEnqueue(tabs, opts, f.Text(), size, f.Offsets(), f.n, 1, nullptr, nullptr, dSpans, f.cap, f.dCounts, f.stream))
			return rc;
	}
	// (the pass reads min(*count, cap) spans: what lies beyond match_cap stays as it is)
	if (int rc = LaunchSplice(f.dRaw, size, dSpans, f.dCounts, f.cap, head, head_len, tail, tail_len, mode & PIRE_HIP_SPLICE_KEEP, nullptr, 0, dOutText,
	                          room, dPos, nullptr, dBytes, kSpliceTotalUnknown, f.stream))
		return rc;
	if (int rc = f.Close("hipMemcpy(splice)"))
		return rc;
	if (f.onDevice)
		return PIRE_HIP_OK;
	if (int rc = HitsBack(1, out_match_count, f.cap, f.cap, out_pos ? dPos : nullptr, out_pos, 8, "hipMemcpy(splice)"))
		return rc;
	if (const uint64_t bytes = std::min(*out_bytes, room)) {
		const hipError_t e = hipMemcpy(out_text, dOutText, size_t(bytes), hipMemcpyDeviceToHost);
		if (e != hipSuccess)
			return HipFail(e, "hipMemcpy(splice)");
	}
	return PIRE_HIP_OK;
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_step(pire_hip_table* t, uint32_t* state_idx, uint64_t n, uint32_t ch, void* stream)
try {
	if (!t || (n && !state_idx) || ch >= kMaxCharUnaligned || ch == kEpsilon) {
		SetError("bad argument");
		return PIRE_HIP_EINVAL;
	}
	ScanParams p;
	TableUse use(t, /*enqueueOnly=*/true);   // device arrays: the call only enqueues
	if (int rc = FillParams(t, &p, 0))
		return rc;
	return LaunchStep(p, state_idx, n, t->host.cls[ch], static_cast<hipStream_t>(stream));
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

int pire_hip_host_alloc(size_t bytes, void** out)
try {
	if (!out) {
		SetError("null out pointer");
		return PIRE_HIP_EINVAL;
	}
	*out = nullptr;
	hipError_t e = hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault);
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipHostMalloc");
} catch (...) {
	return pirehip::HandleException();
}

void pire_hip_host_free(void* p)
{
	if (p)
		(void)hipHostFree(p);
}

int pire_hip_device_alloc(size_t bytes, void** out)
try {
	if (!out) {
		SetError("null out pointer");
		return PIRE_HIP_EINVAL;
	}
	*out = nullptr;
	hipError_t e = hipMalloc(out, bytes ? bytes : 16);
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMalloc");
} catch (...) {
	return pirehip::HandleException();
}

void pire_hip_device_free(void* p)
{
	if (p)
		(void)hipFree(p);
}

int pire_hip_copy_to_device(void* dst_device, const void* src_host, size_t bytes, void* stream)
try {
	hipError_t e = bytes ? hipMemcpyAsync(dst_device, src_host, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream))
	                     : hipSuccess;
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemcpyAsync(H2D)");
} catch (...) {
	return pirehip::HandleException();
}

int pire_hip_copy_to_host(void* dst_host, const void* src_device, size_t bytes, void* stream)
try {
	hipError_t e = bytes ? hipMemcpyAsync(dst_host, src_device, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream))
	                     : hipSuccess;
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemcpyAsync(D2H)");
} catch (...) {
	return pirehip::HandleException();
}

int pire_hip_memset_device(void* dst_device, int value, size_t bytes, void* stream)
try {
	hipError_t e = bytes ? hipMemsetAsync(dst_device, value, bytes, static_cast<hipStream_t>(stream)) : hipSuccess;
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemsetAsync");
} catch (...) {
	return pirehip::HandleException();
}

int pire_hip_stream_synchronize(void* stream)
try {
	hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipStreamSynchronize");
} catch (...) {
	return pirehip::HandleException();
}

int pire_hip_corpus_fill(void* device_out, uint64_t seed, uint64_t first, uint64_t count, uint64_t len,
                         uint64_t stride, const void* plants, void* stream)
try {
	if (!device_out && count && len) {
		SetError("null output");
		return PIRE_HIP_EINVAL;
	}
	return LaunchCorpusFill(static_cast<uint8_t*>(device_out), seed, first, count, len, stride, plants,
	                        static_cast<hipStream_t>(stream));
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}

}  // extern "C"
