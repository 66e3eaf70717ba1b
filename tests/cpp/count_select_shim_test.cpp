// Select() / RunLines() of HalfFinalBatchRunner and CountingBatchRunner (include/pire_hip/batch_runner.hpp) as far as they are
// decided before a device is touched: what the library refuses comes back as Pire::Error with the entry point's name in it,
// and a batch of no strings or no bytes answers zeros.  Scanners built as shim_test.cpp builds them, against the unmodified
// reference headers; into oracle/_ref/bin with the libraries it links.  It needs no GPU and is run without one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire/extra.h>
#include <pire_hip/batch_runner.hpp>

static int g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static Pire::Fsm Parse(const char* re)
{
	return Pire::Lexer(re, re + strlen(re)).Parse();
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

template <class Runner>
static void TestRunner(Runner& gpu, size_t regexps, const char* runName, const char* linesName)
{
	const std::vector<uint64_t> zeros(regexps, 0);
	const std::vector<Pire::ystring> none;
	// no strings: zeros, for every way of asking
	gpu.Begin().Run(none).End().Select();
	CHECK(gpu.HitCount() == 0 && gpu.Hits().empty() && gpu.HitResults().empty() && gpu.Totals() == zeros);
	gpu.Select(std::vector<uint32_t>(regexps, 2), true);
	CHECK(gpu.HitCount() == 0 && gpu.Hits().empty() && gpu.Totals() == zeros);
	CHECK(Thrown([&] { gpu.HitSpans(); }).find("follows RunLines()") != std::string::npos);
	CHECK(Thrown([&] { gpu.LineCount(); }).find("follows RunLines()") != std::string::npos);
	// no bytes: zeros, and no lines
	gpu.RunLines("", 0);
	CHECK(gpu.LineCount() == 0 && gpu.HitCount() == 0 && gpu.Hits().empty() && gpu.HitSpans().empty() && gpu.HitResults().empty());
	CHECK(gpu.Totals() == zeros);
	CHECK(Thrown([&] { gpu.Results(); }).find("RunLines() has hits") != std::string::npos);
	// one threshold per regexp
	gpu.Run(none).Select(std::vector<uint32_t>(regexps + 1, 1));
	CHECK(Thrown([&] { gpu.HitCount(); }).find("one threshold per regexp") != std::string::npos);
	gpu.Select();
	CHECK(gpu.HitCount() == 0);
	// what the library refuses before it touches a device: bytes announced and not given, strings without offsets
	gpu.RunLines(nullptr, 5);
	std::string what = Thrown([&] { gpu.HitCount(); });
	CHECK(what.find(linesName) != std::string::npos && what.find("size > 0 with null raw") != std::string::npos);
	gpu.Run("abc", nullptr, 2);
	what = Thrown([&] { gpu.Hits(); });
	CHECK(what.find(runName) != std::string::npos && what.find("argument") != std::string::npos);
	gpu.Run(none);
	CHECK(gpu.HitCount() == 0 && gpu.Totals() == zeros);
}

template <class CountScanner>
static void TestCounting()
{
	const char* res[] = {"[a-z]+", "http", "abc"};
	const char* seps[] = {"\\s", ".*", ".*"};
	CountScanner glued;
	for (int k = 0; k < 3; ++k) {
		CountScanner one(Parse(res[k]), Parse(seps[k]));
		glued = k == 0 ? one : CountScanner::Glue(glued, one);
	}
	CHECK(glued.RegexpsCount() == 3);
	Pire::Hip::CountingBatchRunner<CountScanner> gpu(glued);
	TestRunner(gpu, 3, "pire_hip_counting_run_select", "pire_hip_counting_lines_select");
}

static void TestHalfFinal()
{
	const Pire::Fsm re = Parse("ab+c|b");
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
	Pire::Hip::HalfFinalBatchRunner<> gpu(glued);
	TestRunner(gpu, 2, "pire_hip_run_half_final_select", "pire_hip_half_final_lines_select");
}

int main()
{
	// the C ABI itself, as a caller in C++ sees it: codes and names
	uint64_t count = 77;
	const uint32_t rows[6] = {1, 0, 0, 2, 3, 0};
	CHECK(pire_hip_count_select(rows, 3, 2, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_count_select: null out_hit_count") == 0);
	CHECK(pire_hip_count_select(rows, 3, 2, nullptr, 2, 0, nullptr, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_count_select(nullptr, 3, 2, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_count_select(rows, 3, 2, nullptr, PIRE_HIP_COUNT_ALL, 0, nullptr, nullptr, nullptr, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_count_select(rows, uint64_t(1) << 32, 2, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EUNSUPPORTED);
	CHECK(pire_hip_count_select(rows, 1, 1025, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EUNSUPPORTED);
	CHECK(count == 77);
	uint64_t totals[2] = {5, 5};
	CHECK(pire_hip_count_select(nullptr, 0, 2, nullptr, 0, 0, totals, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_OK);
	CHECK(count == 0 && totals[0] == 0 && totals[1] == 0);
	try {
		TestCounting<Pire::CountingScanner>();
		TestCounting<Pire::AdvancedCountingScanner>();
		TestCounting<Pire::NoGlueLimitCountingScanner>();
		TestHalfFinal();
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	if (g_fail) {
		fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(count select shim: %d checks)\n", g_checks);
	return 0;
}
