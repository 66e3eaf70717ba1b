// Context() of BatchRunner, SlowBatchRunner and LineMatcher (include/pire_hip/batch_runner.hpp) as far as it is decided before a
// device is touched: what the library refuses comes back as Pire::Error with the entry point's name in it, a buffer of no bytes
// answers zeros, and Context() after anything but RunLines() throws.  Fsms built as easy.h builds them, against the unmodified
// reference headers; into oracle/_ref/bin with the libraries it links.  It needs no GPU and is run without one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire_hip/batch_runner.hpp>

static int g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

// easy.h:205-209: the pattern anywhere in the string
static Pire::Fsm Surrounded(const char* re)
{
	Pire::Fsm fsm = Pire::Lexer(re, re + strlen(re)).Parse();
	fsm.PrependAnything();
	fsm.AppendAnything();
	return fsm;
}

// what `call` throws: the message of the Pire::Error, "" where nothing was thrown
template <class F>
static std::string Thrown(F call)
{
	try {
		call();
	} catch (const Pire::Error& e) {
		return e.what();
	}
	return std::string();
}

static bool Has(const std::string& s, const char* part)
{
	return s.find(part) != std::string::npos;
}

// a runner with a buffer of no bytes behind RunLines() and a Context(): zeros from every accessor
template <class Runner>
static void CheckEmpty(Runner& run)
{
	CHECK(run.ContextLines().empty() && run.ContextFlags().empty() && run.ContextSpans().empty());
	CHECK(run.ContextGroupCount() == 0);
	CHECK(run.ContextText().empty() && run.ContextTextOffsets().size() == 1 && run.ContextTextOffsets()[0] == 0);
	CHECK(run.ContextText('|').empty());
}

static void TestFastRunner()
{
	const Pire::Scanner sc = Surrounded("a.{3}b").Compile<Pire::Scanner>();
	Pire::Hip::BatchRunner<Pire::Scanner> gpu(sc);
	const std::vector<Pire::ystring> none;
	// Context() follows RunLines(), and nothing else
	CHECK(Has(Thrown([&] { gpu.Context(1, 1); }), "Context() follows RunLines()"));
	gpu.Begin().Run(none).End();
	CHECK(Has(Thrown([&] { gpu.Context(1, 1); }), "Context() follows RunLines()"));
	gpu.Begin().RunLinesField("", 0, 1).End();
	CHECK(Has(Thrown([&] { gpu.Context(1, 1); }), "Context() follows RunLines()"));
	// the accessors follow Context()
	gpu.Begin().RunLines("", 0).End();
	CHECK(Has(Thrown([&] { gpu.ContextLines(); }), "ContextLines() follows Context()"));
	CHECK(Has(Thrown([&] { gpu.ContextText(); }), "ContextText() follows Context()"));
	CHECK(Has(Thrown([&] { gpu.ContextTextOffsets(); }), "ContextTextOffsets() follows Context()"));
	// no bytes: no lines, no text -- whatever the window
	gpu.Context(2, 3);
	CheckEmpty(gpu);
	gpu.Context(~uint64_t(0), ~uint64_t(0));
	CheckEmpty(gpu);
	// a selection keeps the request, a batch ends it
	gpu.Select();
	CheckEmpty(gpu);
	gpu.Begin().RunLines("", 0).End();
	CHECK(Has(Thrown([&] { gpu.ContextFlags(); }), "ContextFlags() follows Context()"));
	// what the library refuses before it touches a device
	gpu.Begin().RunLines(nullptr, 5).End().Context(1, 1);
	std::string what = Thrown([&] { gpu.ContextLines(); });
	CHECK(Has(what, "pire_hip_run_lines_context_select") && Has(what, "size > 0 with null raw"));
	what = Thrown([&] { gpu.ContextText(); });
	CHECK(Has(what, "pire_hip_run_lines_context_gather") && Has(what, "size > 0 with null raw"));
	// the hit accessors of RunLines() are what they were
	gpu.Begin().RunLines("", 0).End().Context(1, 1);
	CHECK(gpu.LineCount() == 0 && gpu.HitCount() == 0 && gpu.HitText().empty());
	CheckEmpty(gpu);
}

static void TestSlowRunner()
{
	const Pire::SlowScanner sc = Surrounded("a.{20}$").Compile<Pire::SlowScanner>();
	Pire::Hip::SlowBatchRunner gpu(sc);
	const std::vector<Pire::ystring> none;
	CHECK(Has(Thrown([&] { gpu.Context(1, 1); }), "Context() follows RunLines()"));
	gpu.Run(none);
	CHECK(Has(Thrown([&] { gpu.Context(1, 1); }), "Context() follows RunLines()"));
	for (int invert = 0; invert < 2; ++invert) {
		gpu.RunLines("", 0, '\n', invert != 0);
		CHECK(Has(Thrown([&] { gpu.ContextSpans(); }), "ContextSpans() follows Context()"));
		gpu.Context(0, 4);
		CheckEmpty(gpu);
		gpu.Select(invert == 0);   // (honoured: the request stays, the lists are fetched anew)
		CheckEmpty(gpu);
	}
	gpu.RunLines(nullptr, 5).Context(1, 1);
	std::string what = Thrown([&] { gpu.ContextGroupCount(); });
	CHECK(Has(what, "pire_hip_slow_lines_context_select") && Has(what, "size > 0 with null raw"));
	what = Thrown([&] { gpu.ContextTextOffsets(); });
	CHECK(Has(what, "pire_hip_slow_lines_context_gather") && Has(what, "size > 0 with null raw"));
}

static void TestLineMatcher()
{
	Pire::Hip::LineMatcher fast(Surrounded("a.{3}b"));
	Pire::Hip::LineMatcher slow(Surrounded("a.{20}$"));   // 2^21 subsets: Fsm::Determine() gives up
	CHECK(!fast.IsSlow() && slow.IsSlow());
	Pire::Hip::LineMatcher* both[2] = {&fast, &slow};
	for (int k = 0; k < 2; ++k) {
		Pire::Hip::LineMatcher& m = *both[k];
		CHECK(Has(Thrown([&] { m.Context(1, 1); }), "Context() follows RunLines()"));
		m.RunLines("", 0).Context(1, 2);
		CheckEmpty(m);
		m.RunLines(nullptr, 5).Context(1, 2);
		CHECK(Has(Thrown([&] { m.ContextLines(); }), "size > 0 with null raw"));
		CHECK(Has(Thrown([&] { m.ContextText(); }), "size > 0 with null raw"));
	}
	slow.RunLines("", 0, '\n', true).Context(3, 0);
	CheckEmpty(slow);
}

int main()
{
	// the C ABI itself, as a caller in C++ sees it: codes and names
	uint64_t count = 77, groups = 77, lines = 77, hitCount = 77, bytes = 77;
	uint64_t out[4] = {9, 9, 9, 9};
	uint8_t flags[4] = {9, 9, 9, 9};
	const uint64_t hits[3] = {1, 4, 6}, unsorted[3] = {4, 1, 6}, twice[3] = {1, 1, 6};
	CHECK(pire_hip_context(hits, nullptr, 3, 8, 1, 1, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_context: null out_line_count") == 0);
	CHECK(pire_hip_context(nullptr, nullptr, 3, 8, 1, 1, 0, nullptr, nullptr, 0, &count, nullptr, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_context: hit_cap > 0 with null hits") == 0);
	CHECK(pire_hip_context(hits, nullptr, 3, 8, 1, 1, 0, nullptr, nullptr, 4, &count, nullptr, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_context: line_cap > 0 with null out_lines") == 0);
	CHECK(pire_hip_context(hits, nullptr, 3, 8, 1, 1, 0, nullptr, flags, 0, &count, nullptr, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_context: out_line_flags without out_lines") == 0);
	CHECK(pire_hip_context(hits, nullptr, 3, uint64_t(1) << 32, 1, 1, 0, out, flags, 4, &count, &groups, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_context(hits, nullptr, uint64_t(1) << 32, 8, 1, 1, 0, out, flags, 4, &count, &groups, nullptr) == PIRE_HIP_EINVAL);
	// host pointers: the list is looked at before anything is written
	CHECK(pire_hip_context(unsorted, nullptr, 3, 8, 1, 1, 0, out, flags, 4, &count, &groups, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_context: hits must be strictly ascending") == 0);
	CHECK(pire_hip_context(twice, nullptr, 3, 8, 1, 1, 0, out, flags, 4, &count, &groups, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_context(hits, nullptr, 3, 6, 1, 1, 0, out, flags, 4, &count, &groups, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_context: hit out of range") == 0);
	CHECK(count == 77 && groups == 77 && out[0] == 9 && flags[0] == 9);
	// no lines or no hits: zeros, no device is touched (a hit_count of 0 counts)
	const uint64_t zero = 0;
	CHECK(pire_hip_context(hits, &zero, 3, 8, 1, 1, 0, out, flags, 4, &count, &groups, nullptr) == PIRE_HIP_OK);
	CHECK(count == 0 && groups == 0 && out[0] == 9 && flags[0] == 9);
	count = groups = 77;
	CHECK(pire_hip_context(nullptr, nullptr, 0, 0, 1, 1, 0, nullptr, nullptr, 0, &count, nullptr, nullptr) == PIRE_HIP_OK);
	CHECK(count == 0 && groups == 77);
	// the lines forms
	CHECK(pire_hip_run_lines_context_select(nullptr, "a\n", 2, '\n', 0, nullptr, 1, 1, &lines, nullptr, nullptr, nullptr, 0, &count, nullptr,
	                                        nullptr, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_run_lines_context_select: null table") == 0);
	CHECK(pire_hip_slow_lines_context_gather(nullptr, "a\n", 2, '\n', 0, 0, 1, 1, &lines, nullptr, nullptr, nullptr, 0, &count, &groups,
	                                         &hitCount, '\n', nullptr, 0, nullptr, &bytes, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_slow_lines_context_gather: null table") == 0);
	CHECK(lines == 77 && hitCount == 77 && bytes == 77);
	try {
		TestFastRunner();
		TestSlowRunner();
		TestLineMatcher();
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	if (g_fail) {
		fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(context shim: %d checks)\n", g_checks);
	return 0;
}
