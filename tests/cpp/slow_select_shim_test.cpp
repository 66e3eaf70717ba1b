// Select() / RunLines() of SlowBatchRunner and the choice LineMatcher makes (include/pire_hip/batch_runner.hpp) as far as they
// are decided before a device is touched: what the library refuses comes back as Pire::Error with the entry point's name in
// it, a batch of no strings or no bytes answers zeros, and a pattern that does not determinise gets the SlowScanner.  Fsms
// built as easy.h builds them, against the unmodified reference headers; into oracle/_ref/bin with the libraries it links.
// It needs no GPU and is run without one.
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

static void TestSlowRunner()
{
	const Pire::SlowScanner sc = Surrounded("a.{20}$").Compile<Pire::SlowScanner>();
	Pire::Hip::SlowBatchRunner gpu(sc);
	const std::vector<Pire::ystring> none;
	CHECK(Has(Thrown([&] { gpu.Hits(); }), "follows Run() or RunLines()"));
	// no strings: zeros, in both modes
	gpu.Run(none).Select();
	CHECK(gpu.HitCount() == 0 && gpu.Hits().empty());
	gpu.Select(true);
	CHECK(gpu.HitCount() == 0 && gpu.Hits().empty());
	CHECK(Has(Thrown([&] { gpu.HitSpans(); }), "HitSpans() follows RunLines()"));
	CHECK(Has(Thrown([&] { gpu.LineCount(); }), "LineCount() follows RunLines()"));
	CHECK(Has(Thrown([&] { gpu.HitText(); }), "HitText() follows RunLines()"));
	// no bytes: no lines, no hits, no text
	for (int invert = 0; invert < 2; ++invert) {
		gpu.RunLines("", 0, '\n', invert != 0);
		CHECK(gpu.LineCount() == 0 && gpu.HitCount() == 0 && gpu.Hits().empty() && gpu.HitSpans().empty());
		CHECK(gpu.HitText().empty() && gpu.HitTextOffsets().size() == 1 && gpu.HitTextOffsets()[0] == 0);
	}
	// what the library refuses before it touches a device: bytes announced and not given, strings without offsets
	gpu.RunLines(nullptr, 5);
	std::string what = Thrown([&] { gpu.HitCount(); });
	CHECK(Has(what, "pire_hip_slow_lines_select") && Has(what, "size > 0 with null raw"));
	what = Thrown([&] { gpu.HitText(); });
	CHECK(Has(what, "pire_hip_slow_lines_gather") && Has(what, "size > 0 with null raw"));
	gpu.Run("abc", nullptr, 2);
	what = Thrown([&] { gpu.Hits(); });
	CHECK(Has(what, "pire_hip_slow_run_select") && Has(what, "null offsets"));
	gpu.Run(none);
	CHECK(gpu.HitCount() == 0);
}

static void TestLineMatcher()
{
	Pire::Hip::LineMatcher fast(Surrounded("a.{3}b"));
	CHECK(!fast.IsSlow());
	Pire::Hip::LineMatcher slow(Surrounded("a.{20}$"));   // 2^21 subsets: Fsm::Determine() gives up
	CHECK(slow.IsSlow());
	Pire::Hip::LineMatcher* both[2] = {&fast, &slow};
	for (int k = 0; k < 2; ++k) {
		Pire::Hip::LineMatcher& m = *both[k];
		m.RunLines("", 0);
		CHECK(m.LineCount() == 0 && m.HitCount() == 0 && m.Hits().empty() && m.HitSpans().empty());
		CHECK(m.HitText().empty() && m.HitTextOffsets().size() == 1);
		m.RunLines(nullptr, 5);
		CHECK(Has(Thrown([&] { m.HitCount(); }), "size > 0 with null raw"));
		CHECK(Has(Thrown([&] { m.HitText(); }), "size > 0 with null raw"));
	}
	// the inverted selection is the SlowScanner's
	slow.RunLines("", 0, '\n', true);
	CHECK(slow.HitCount() == 0 && slow.HitText().empty());
	CHECK(Has(Thrown([&] { fast.RunLines("", 0, '\n', true); }), "inverted selection"));
}

int main()
{
	// the C ABI itself, as a caller in C++ sees it: codes and names
	uint64_t count = 77, lines = 77, bytes = 77;
	uint64_t hits[4] = {9, 9, 9, 9};
	const uint8_t fin[3] = {1, 0, 2};
	CHECK(pire_hip_final_select(fin, 3, 0, 0, nullptr, 0, nullptr, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_final_select: null out_hit_count") == 0);
	CHECK(pire_hip_final_select(fin, 3, 2, 0, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_final_select(nullptr, 3, 0, 0, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_final_select(fin, 3, PIRE_HIP_FINAL_SELECT_ZERO, 0, nullptr, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_final_select(fin, uint64_t(1) << 32, 0, 0, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(count == 77);
	CHECK(pire_hip_final_select(nullptr, 0, PIRE_HIP_FINAL_SELECT_ZERO, 0, hits, 4, &count, nullptr) == PIRE_HIP_OK);
	CHECK(count == 0 && hits[0] == 9);
	CHECK(pire_hip_slow_lines_select(nullptr, "a\n", 2, '\n', 0, 0, &lines, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_slow_lines_select: null table") == 0);
	CHECK(pire_hip_slow_lines_gather(nullptr, "a\n", 2, '\n', 0, 0, '\n', &lines, nullptr, 0, &count, nullptr, 0, nullptr, &bytes, nullptr) ==
	      PIRE_HIP_EINVAL);
	CHECK(lines == 77 && bytes == 77);
	try {
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
	printf("OK(slow select shim: %d checks)\n", g_checks);
	return 0;
}
