// Which C calls include/pire_hip/batch_runner.hpp makes, in which order and with which arguments, for every runner and every
// form of asking -- recorded by the stand-in tests/cpp/recording_hip.cpp (no library, no device) into the file named on the
// command line, which tests/test_shim_calls.py compares byte for byte with tests/cpp/shim_calls.expected.txt.  Scanners built
// as shim_test.cpp and count_select_shim_test.cpp build them, against the unmodified reference headers.  The checks here are
// the shaped results the header leaves: vector sizes after a shrink, exceptions and their texts.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire/extra.h>
#include <pire_hip/batch_runner.hpp>

// the stand-in's script (recording_hip.cpp)
extern FILE* g_rec_out;
extern uint32_t g_rec_regexps;
extern uint64_t g_rec_hit_count, g_rec_line_count, g_rec_bytes;
extern std::vector<uint64_t> g_rec_route_counts;
extern int g_rec_fail_next;
void rec_note(const char* fmt, ...);

static int g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static Pire::Fsm Parse(const char* re, bool surround = true)
{
	Pire::Fsm fsm = Pire::Lexer(re, re + strlen(re)).Parse();
	if (surround)
		fsm.Surround();
	return fsm;
}

// what `call` throws: the message of the Pire::Error, "" where nothing was thrown (into the trace as well)
template <class F>
static std::string Thrown(F call)
{
	std::string what;
	try {
		call();
	} catch (const Pire::Error& e) {
		what = e.what();
	}
	rec_note("thrown: %s", what.c_str());
	return what;
}

static void Script(uint64_t hits, uint64_t lines = 0, uint64_t bytes = 0)
{
	g_rec_hit_count = hits;
	g_rec_line_count = lines;
	g_rec_bytes = bytes;
}

static const std::vector<Pire::ystring> kStrings = {"aaa", "bbb", "", "aaabbb"};
static const char kFlat[] = "aaabbbaaabbb";
static const uint64_t kOffsets[5] = {0, 3, 6, 6, 12};
static const char kRaw[] = "aaa\nbbb\n\nx\taaa\ty\n";
static const size_t kRawSize = sizeof(kRaw) - 1;
static const size_t kFirstCap = kRawSize / 64 + 1024;     // what the lines forms of BatchRunner and CaptureBatchRunner start with

static Pire::Scanner Glued()
{
	return Pire::Scanner::Glue(Parse("aaa").Compile<Pire::Scanner>(), Parse("bbb").Compile<Pire::Scanner>());
}

static void TestBatchRunnerOnHost(const Pire::Scanner& sc)
{
	rec_note("BatchRunner: host pointers");
	g_rec_regexps = 2;
	Pire::Hip::BatchRunner<Pire::Scanner> run(sc);
	run.Begin().Run(kFlat, kOffsets, 4).End();
	CHECK(run.States().size() == 4 && run.Finals().size() == 4 && run.MatchCounts().size() == 4);
	CHECK(run.Flags() == (PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END));
	rec_note("From(), Run(vector)");
	const std::vector<Pire::Scanner::State> mid = run.States();
	run.From(mid).Run(kStrings);
	CHECK(run.States().size() == 4);
	CHECK(Thrown([&] { run.Run(kFlat, kOffsets, 3).States(); }).find("From() and Run() disagree") != std::string::npos);
	run.From(std::vector<Pire::Scanner::State>());
	rec_note("n == 0, with and without offsets");
	run.Run(kFlat, nullptr, 0);
	CHECK(run.States().empty() && run.MatchCounts().size() == 4);
	run.Run(std::vector<Pire::ystring>());
	CHECK(run.Finals().empty());
	CHECK(run.Select().HitCount() == 0);
	CHECK(run.Route().RouteCount(1) == 0);
	rec_note("Select(): Hits() then HitMasks() is one select");
	Script(3);
	run.Run(kStrings).Select();
	CHECK(run.Hits().size() == 3 && run.HitMasks().size() == 3 && run.HitCount() == 3);
	rec_note("Select({1}) after Hits() selects again and does not scan again");
	Script(2);
	run.Select({1});
	CHECK(run.HitMasks().size() == 2 && run.Hits().size() == 2);
	run.Select({0, 1, 70});                                   // (a regexp beyond the mask is dropped)
	CHECK(run.HitCount() == 2);
	rec_note("a new Run after Select(): scan and select again, with the same want");
	run.Run(kFlat, kOffsets, 4);
	CHECK(run.Hits().size() == 2);
	rec_note("as it is: a new Run whose States() are asked first keeps the selection of the batch before");
	run.Run(kStrings);
	CHECK(run.States().size() == 4 && run.Hits().size() == 2);
	rec_note("Hits() with no Select() at all");
	Pire::Hip::BatchRunner<Pire::Scanner> fresh(run.GetTable());
	CHECK(fresh.Begin().Run(kStrings).End().Hits().size() == 2);
	CHECK(Thrown([&] { fresh.HitText(); }).find("HitText() follows RunLines()") != std::string::npos);
	CHECK(Thrown([&] { fresh.RouteSpans(0); }).find("RouteSpans() follows RunLines()") != std::string::npos);
	rec_note("Route() on host: after a scan that was made, and on a new batch");
	g_rec_route_counts = {2, 1};
	CHECK(fresh.Route().RouteCount(0) == 2 && fresh.RouteHits(0).size() == 2 && fresh.RouteHits(1).size() == 1);
	CHECK(fresh.RoutePitch() == 4);
	fresh.Run(kFlat, kOffsets, 2);
	g_rec_route_counts = {1, 2};
	CHECK(fresh.RouteHits(1).size() == 2 && fresh.RouteCount(0) == 1);
	fresh.Route();
	CHECK(fresh.RouteCount(1) == 2 && fresh.States().size() == 2);
	rec_note("a refusal of the library is a Pire::Error");
	g_rec_fail_next = 1;
	CHECK(Thrown([&] { fresh.Run(kStrings).States(); }) == "pire_hip: recording_hip: scripted refusal");
	CHECK(fresh.States().size() == 4);
	rec_note("Adapt(), FreezeRanking()");
	Pire::Hip::Table<Pire::Scanner> table(sc);
	CHECK(table.Adapt() == 3);
	Pire::Hip::Table<Pire::Scanner>::FreezeRanking(true);
	rec_note("the runners go");
}

static void TestBatchRunnerOnDevice(const Pire::Scanner& sc)
{
	rec_note("BatchRunner: device pointers");
	g_rec_regexps = 2;
	g_rec_route_counts = {2, 1};
	int stream = 0;
	Pire::Hip::BatchRunner<Pire::Scanner> run(sc);
	run.Begin().RunDevice(kFlat, kOffsets, 4, &stream).End();
	CHECK(run.DeviceStateIndices() != nullptr && run.DeviceFinals() != nullptr);
	CHECK(run.States().size() == 4 && run.Finals().size() == 4);
	CHECK(run.MatchCounts().size() == 4 && run.MatchCounts()[0] == 4);
	rec_note("From() on device");
	const std::vector<Pire::Scanner::State> mid = run.States();
	run.From(mid).RunDevice(kFlat, kOffsets, 4);
	CHECK(run.MatchCounts().size() == 4 && run.States().size() == 4);
	run.From(std::vector<Pire::Scanner::State>());
	rec_note("Select() on device, without and with regexps");
	Script(3);
	run.RunDevice(kFlat, kOffsets, 4, &stream);
	CHECK(run.DeviceHits() != nullptr && run.DeviceHitMasks() != nullptr && run.DeviceHitCount() != nullptr);
	CHECK(run.Hits().size() == 3 && run.HitMasks().size() == 3);
	run.Select({0});
	CHECK(run.HitCount() == 3 && run.DeviceHits() != nullptr);
	Script(0);
	run.Select();
	CHECK(run.Hits().empty());
	rec_note("Route() on device");
	CHECK(run.Route().DeviceRouteHits() != nullptr && run.DeviceRouteCounts() != nullptr && run.RoutePitch() == 4);
	CHECK(run.RouteHits(0).size() == 2 && run.RouteCount(1) == 1);
	rec_note("RunDeviceStrided, and n == 0 on device");
	run.RunDeviceStrided(kFlat, 4, 2, 3, &stream);
	CHECK(run.Finals().size() == 4 && run.HitCount() == 0);
	run.RunDeviceStrided(kFlat, 0, 2, 3);
	CHECK(run.States().empty() && run.Route().RouteCount(0) == 2);
	rec_note("as it is: RunDevice() with no offsets and n > 0 is scanned as n records of no bytes");
	run.RunDevice(kFlat, nullptr, 3, &stream);
	CHECK(run.States().size() == 3 && run.MatchCounts()[0] == 3);
	rec_note("the runner goes");
}

static void TestBatchRunnerLines(const Pire::Scanner& sc)
{
	rec_note("BatchRunner: RunLines");
	g_rec_regexps = 2;
	Pire::Hip::BatchRunner<Pire::Scanner> run(sc);
	Script(2, 4, 8);
	run.Begin().RunLines(kRaw, kRawSize).End();
	CHECK(run.Hits().size() == 2 && run.HitSpans().size() == 4 && run.HitMasks().size() == 2 && run.LineCount() == 4 && run.HitCount() == 2);
	CHECK(Thrown([&] { run.States(); }) == "pire_hip: RunLines() has hits, no states");
	CHECK(Thrown([&] { run.MatchCounts(); }) == "pire_hip: RunLines() has hits, no states");
	rec_note("HitText() after Hits() scans a second time with cap = HitCount(); another tail fetches again");
	CHECK(run.HitText().size() == 8 && run.HitTextOffsets().size() == 3);
	CHECK(run.HitText().size() == 8);
	CHECK(run.HitText('\0').size() == 8 && run.HitTextOffsets().size() == 3);
	rec_note("one retry: more hits than the first capacity");
	Script(kFirstCap + 5, 4000, 8);
	run.RunLines(kRaw, kRawSize, ';');
	CHECK(run.Hits().size() == kFirstCap + 5 && run.HitSpans().size() == 2 * (kFirstCap + 5) && run.HitMasks().size() == kFirstCap + 5);
	rec_note("HitTextOffsets() alone implies '\\n'; one retry there as well");
	run.RunLines(kRaw, kRawSize);
	CHECK(run.HitTextOffsets().size() == kFirstCap + 6 && run.HitText().size() == 8);
	rec_note("Select({0}) after the text: both are fetched again");
	Script(1, 4, 4);
	run.Select({0});
	CHECK(run.HitText().size() == 4 && run.Hits().size() == 1 && run.DeviceHits() == nullptr);
	rec_note("RunLinesField, with rest");
	run.RunLinesField(kRaw, kRawSize, 1);
	CHECK(run.HitCount() == 1 && run.HitText('\t').size() == 4);
	run.RunLinesField(kRaw, kRawSize, 2, ',', ';', true);
	CHECK(run.HitTextOffsets().size() == 2 && run.HitSpans().size() == 2);
	CHECK(Thrown([&] { run.Route().RouteCount(0); }) == "pire_hip: Route() follows Run*() or RunLines(), not RunLinesField()");
	rec_note("Route() after RunLines, with one retry; then Hits(); and the reverse order");
	g_rec_route_counts = {kFirstCap + 3, 1};
	run.RunLines(kRaw, kRawSize);
	CHECK(run.Route().RouteHits(0).size() == kFirstCap + 3 && run.RouteSpans(1).size() == 2 && run.RoutePitch() == kFirstCap + 3);
	CHECK(run.Hits().size() == 1 && run.RouteCount(1) == 1);
	g_rec_route_counts = {1, 2};
	run.RunLines(kRaw, kRawSize);
	CHECK(run.Hits().size() == 1 && run.RouteSpans(1).size() == 4 && run.LineCount() == 4);
	rec_note("a plain Run after the lines");
	run.Run(kStrings);
	CHECK(run.States().size() == 4 && run.Hits().size() == 1 && run.RouteHits(1).size() == 2);
	rec_note("no bytes");
	Script(0);
	run.RunLines(nullptr, 0);
	CHECK(run.Hits().empty() && run.HitText().empty() && run.HitTextOffsets().size() == 1);
	rec_note("the runner goes");
}

static void TestPairMultiPrefixSlow(const Pire::Scanner& sc)
{
	rec_note("PairBatchRunner: host, then fused strided");
	g_rec_regexps = 1;
	Script(0);
	Pire::SimpleScanner s2 = Parse("abc|def").Compile<Pire::SimpleScanner>();
	{
		Pire::Hip::PairBatchRunner<Pire::Scanner, Pire::SimpleScanner> pair(sc, s2);
		pair.Begin().Run(kFlat, kOffsets, 4).End();
		CHECK(pair.States().size() == 4 && pair.Finals().size() == 4);
		pair.Run(kStrings);
		CHECK(pair.Finals().size() == 4);
		int stream = 0;
		pair.RunDeviceStrided(kFlat, 4, 2, 3, &stream);
		CHECK(pair.States().size() == 4 && pair.Finals().size() == 4 && pair.Finals()[0] == 1);
		CHECK(pair.First().States().size() == 4);
	}
	rec_note("MultiBatchRunner");
	g_rec_regexps = 2;
	{
		Pire::Hip::MultiBatchRunner<Pire::Scanner> all(sc);
		CHECK(all.Begin().Run(kStrings).End().States().size() == 4 && all.Finals().size() == 4 && all.MatchCounts().size() == 4);
		CHECK(all.Devices() == 2 && std::string(all.Backend()) == "host");
		all.Run(kFlat, nullptr, 0);
		CHECK(all.States().empty());
		Pire::Hip::MultiBatchRunner<Pire::Scanner> two(sc, {0, 1});
		CHECK(two.Run(kFlat, kOffsets, 4).Finals().size() == 4);
	}
	rec_note("prefix, suffix");
	{
		Pire::Hip::Table<Pire::Scanner> table(sc);
		std::vector<const char*> p = Pire::Hip::BatchLongestPrefix(table, kFlat, kOffsets, 4);
		CHECK(p.size() == 4 && p[0] == kFlat + 1 && p[1] == nullptr);
		p = Pire::Hip::BatchShortestPrefix(table, kFlat, kOffsets, 4, true, false);
		CHECK(p.size() == 4);
		CHECK(Pire::Hip::BatchLongestPrefix(table, kFlat, nullptr, 0, false, true).empty());
		p = Pire::Hip::BatchLongestSuffix(table, kFlat, kOffsets, 4);
		CHECK(p.size() == 4 && p[0] == kFlat + 3 - 1 - 1 && p[1] == nullptr);
		p = Pire::Hip::BatchShortestSuffix(table, kFlat, kOffsets, 4, true, false);
		CHECK(p.size() == 4);
		CHECK(Pire::Hip::BatchShortestSuffix(table, kFlat, nullptr, 0, false, true).empty());
	}
	rec_note("SlowBatchRunner");
	{
		Pire::SlowScanner slow = Parse("a.{30}$").Compile<Pire::SlowScanner>();
		Pire::Hip::SlowBatchRunner run(slow);
		CHECK(run.Matches(kFlat, kOffsets, 4).size() == 4);
		CHECK(run.Matches(kFlat, nullptr, 0).empty());
	}
}

template <class Runner>
static void TestCounted(Runner& run, size_t regexps, const char* name)
{
	rec_note("%s", name);
	g_rec_regexps = uint32_t(regexps);
	Script(0);
	run.Begin().Run(kFlat, kOffsets, 4).End();
	CHECK(run.Results().size() == 4 * regexps && run.StateIndices().size() == 4 && run.Result(1, 0) == 7);
	rec_note("Select: no thresholds, thresholds, ALL");
	Script(3);
	CHECK(run.Select().Hits().size() == 3 && run.HitResults().size() == 3 * regexps && run.HitCount() == 3 && run.Totals().size() == regexps);
	std::vector<uint32_t> min(regexps, 0);
	min[0] = 3;
	min[regexps - 1] = 1;
	Script(1);
	CHECK(run.Select(min).HitCount() == 1 && run.Hits().size() == 1);
	CHECK(run.Select(min, true).HitResults().size() == regexps);
	rec_note("one retry: the library reports more hits than strings");
	Script(9);
	CHECK(run.Run(kStrings).Select().Hits().size() == 9 && run.HitResults().size() == 9 * regexps);
	CHECK(Thrown([&] { run.HitSpans(); }) == "pire_hip: HitSpans() follows RunLines()");
	CHECK(Thrown([&] { run.LineCount(); }) == "pire_hip: LineCount() follows RunLines()");
	CHECK(run.Results().size() == 4 * regexps);
	rec_note("n == 0, with and without offsets");
	Script(0);
	CHECK(run.Run(std::vector<Pire::ystring>()).HitCount() == 0 && run.Results().empty());
	CHECK(run.Run(kFlat, nullptr, 0).Hits().empty() && run.StateIndices().empty());
	rec_note("RunLines, then with one retry");
	Script(2, 4);
	run.RunLines(kRaw, kRawSize);
	CHECK(run.HitSpans().size() == 4 && run.LineCount() == 4 && run.Hits().size() == 2 && run.HitResults().size() == 2 * regexps);
	CHECK(Thrown([&] { run.Results(); }) == "pire_hip: RunLines() has hits, no results per string");
	Script(kRawSize / 64 + 16 + 4, 50);
	run.RunLines(kRaw, kRawSize, ';').Select(min, true);
	CHECK(run.Hits().size() == kRawSize / 64 + 20 && run.HitSpans().size() == 2 * (kRawSize / 64 + 20) && run.LineCount() == 50);
	rec_note("a wrong threshold count; no bytes");
	run.Select(std::vector<uint32_t>(regexps + 1, 1));
	CHECK(Thrown([&] { run.HitCount(); }) == "pire_hip: Select() takes one threshold per regexp");
	Script(0);
	run.Select().RunLines(nullptr, 0);
	CHECK(run.Hits().empty() && run.HitSpans().empty() && run.LineCount() == 0);
	rec_note("a refusal of the library");
	g_rec_fail_next = 1;
	CHECK(Thrown([&] { run.Run(kStrings).Hits(); }) == "pire_hip: recording_hip: scripted refusal");
	rec_note("the runner goes");
}

template <class CountScanner>
static void TestCounting(const char* name)
{
	const char* res[] = {"[a-z]+", "http", "abc"};
	const char* seps[] = {"\\s", ".*", ".*"};
	CountScanner glued;
	for (int k = 0; k < 3; ++k) {
		CountScanner one(Parse(res[k], false), Parse(seps[k], false));
		glued = k == 0 ? one : CountScanner::Glue(glued, one);
	}
	CHECK(glued.RegexpsCount() == 3);
	Pire::Hip::CountingBatchRunner<CountScanner> run(glued);
	TestCounted(run, 3, name);
}

static void TestHalfFinal()
{
	const Pire::Fsm re = Parse("ab+c|b", false);
	Pire::HalfFinalScanner glued;
	for (int mode = 0; mode < 2; ++mode) {
		Pire::HalfFinalFsm fsm(re);
		if (mode == 0)
			fsm.MakeGreedyCounter(true);
		else
			fsm.MakeNonGreedyCounter(false);
		Pire::HalfFinalScanner one(fsm);
		glued = mode == 0 ? one : Pire::HalfFinalScanner::Glue(glued, one);
	}
	CHECK(glued.RegexpsCount() == 2);
	Pire::Hip::HalfFinalBatchRunner<> run(glued);
	TestCounted(run, 2, "HalfFinalBatchRunner");
	g_rec_regexps = 2;
	CHECK(run.Run(kStrings).Finals().size() == 4 && run.Finals()[0] == 1);
}

static void TestCapture()
{
	rec_note("CaptureBatchRunner");
	const char* regexp = "id\\s*=\\s*'([a-z0-9]+)'";
	Pire::Lexer lexer;
	lexer.Assign(regexp, regexp + strlen(regexp));
	lexer.AddFeature(Pire::Features::Capture(1));
	Pire::Fsm fsm = lexer.Parse();
	fsm.Surround();
	fsm.Determine();
	Pire::CapturingScanner sc = fsm.Compile<Pire::CapturingScanner>();
	Pire::Hip::CaptureBatchRunner run(sc);
	Script(2);
	run.Begin().Run(kFlat, kOffsets, 4).End();
	CHECK(run.Captured(0) && run.Begin(1) == 2 && run.End(2) == 3 && !run.Final(3) && run.StateIndex(0) == 0);
	rec_note("CapturedLines after the accessors, and before them");
	CHECK(run.CapturedLines().size() == 2 && run.CapturedSpans().size() == 4 && run.LineCount() == 4);
	CHECK(Thrown([&] { run.CapturedText(); }) == "pire_hip: CapturedText() follows RunLines()");
	run.Run(kStrings);
	CHECK(run.CapturedSpans().size() == 4 && run.Captured(3));
	run.Run(kFlat, nullptr, 0);
	CHECK(run.CapturedLines().empty() && run.LineCount() == 0);
	rec_note("RunLines: the list, then the text with cap = the list's length, then a second tail");
	Script(2, 4, 6);
	run.RunLines(kRaw, kRawSize);
	CHECK(run.CapturedLines().size() == 2 && run.CapturedSpans().size() == 4 && run.LineCount() == 4);
	CHECK(run.CapturedText().size() == 6 && run.CapturedTextOffsets().size() == 3);
	CHECK(run.CapturedText().size() == 6);
	CHECK(run.CapturedText(',').size() == 6 && run.CapturedLines().size() == 2);
	CHECK(Thrown([&] { run.Captured(0); }) == "pire_hip: the accessors per string follow Run(), not RunLines()");
	CHECK(Thrown([&] { run.StateIndex(0); }) == "pire_hip: the accessors per string follow Run(), not RunLines()");
	rec_note("one retry of the list; CapturedTextOffsets() alone implies '\\n', one retry");
	Script(kFirstCap + 2, 3000, 6);
	run.RunLines(kRaw, kRawSize, ';');
	CHECK(run.CapturedLines().size() == kFirstCap + 2 && run.CapturedSpans().size() == 2 * (kFirstCap + 2));
	run.RunLines(kRaw, kRawSize);
	CHECK(run.CapturedTextOffsets().size() == kFirstCap + 3 && run.CapturedLines().size() == kFirstCap + 2 && run.CapturedText().size() == 6);
	rec_note("the runner goes");
}

int main(int argc, char** argv)
{
	if (argc != 2) {
		fprintf(stderr, "usage: %s TRACE\n", argv[0]);
		return 2;
	}
	g_rec_out = fopen(argv[1], "w");
	if (!g_rec_out) {
		perror(argv[1]);
		return 2;
	}
	try {
		const Pire::Scanner sc = Glued();
		CHECK(sc.RegexpsCount() == 2);
		TestBatchRunnerOnHost(sc);
		TestBatchRunnerOnDevice(sc);
		TestBatchRunnerLines(sc);
		TestPairMultiPrefixSlow(sc);
		TestCounting<Pire::CountingScanner>("CountingBatchRunner<CountingScanner>");
		TestCounting<Pire::AdvancedCountingScanner>("CountingBatchRunner<AdvancedCountingScanner>");
		TestCounting<Pire::NoGlueLimitCountingScanner>("CountingBatchRunner<NoGlueLimitCountingScanner>");
		TestHalfFinal();
		TestCapture();
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	rec_note("%d checks", g_checks);
	if (fclose(g_rec_out) != 0)
		return 2;
	if (g_fail) {
		fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(shim calls: %d checks)\n", g_checks);
	return 0;
}
