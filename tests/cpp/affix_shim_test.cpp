// AffixBatchRunner (include/pire_hip/batch_runner.hpp) as far as it is decided before a device is touched: what the library
// refuses comes back as Pire::Error with the entry point's name in it, a batch of no strings or no bytes answers zeros, and
// either scanner may be absent.  Scanners built as the reference's own test builds them (pire_ut.cpp:278-306: not surrounded,
// the tail from Fsm::Reverse()), against the unmodified reference headers; into oracle/_ref/bin with the libraries it links.
// It needs no GPU and is run without one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire_hip/batch_runner.hpp>

static int g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static Pire::Scanner Forward(const char* re)
{
	return Pire::Lexer(re, re + strlen(re)).Parse().Compile<Pire::Scanner>();
}

static Pire::Scanner Reversed(const char* re)
{
	return Pire::Lexer(re, re + strlen(re)).Parse().Reverse().Compile<Pire::Scanner>();
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

typedef Pire::Hip::AffixBatchRunner<Pire::Scanner> Runner;

static void TestEmptyBatches(Runner& gpu)
{
	const std::vector<Pire::ystring> none;
	const uint32_t parts[3] = {PIRE_HIP_AFFIX_HEAD, PIRE_HIP_AFFIX_TAIL, PIRE_HIP_AFFIX_REST};
	for (int k = 0; k < 3; ++k) {
		// no strings: zeros
		gpu.Run(none).Select(parts[k]);
		CHECK(gpu.HitCount() == 0 && gpu.Hits().empty() && gpu.Spans().empty());
		CHECK(Has(Thrown([&] { gpu.LineCount(); }), "LineCount() follows RunLines()"));
		CHECK(Has(Thrown([&] { gpu.HitText(); }), "HitText() follows RunLines()"));
		// no bytes: no lines, no hits, no text
		gpu.RunLines("", 0, '\n', parts[k]);
		CHECK(gpu.LineCount() == 0 && gpu.HitCount() == 0 && gpu.Hits().empty() && gpu.Spans().empty());
		CHECK(gpu.HitText().empty() && gpu.HitTextOffsets().size() == 1 && gpu.HitTextOffsets()[0] == 0);
	}
}

static void TestRunner()
{
	const Pire::Scanner head = Forward("[ \\t]+"), tail = Reversed("[ \\t]+");
	const std::vector<Pire::ystring> none;
	Runner both(&head, &tail);
	CHECK(Has(Thrown([&] { both.Hits(); }), "follows Run() or RunLines()"));
	TestEmptyBatches(both);
	// what the library refuses before it touches a device
	both.Run(none).Select(3);
	std::string what = Thrown([&] { both.Hits(); });
	CHECK(Has(what, "pire_hip_affix_run_select") && Has(what, "unknown part"));
	both.RunLines("", 0, '\n', 7);
	what = Thrown([&] { both.HitCount(); });
	CHECK(Has(what, "pire_hip_affix_lines_gather") && Has(what, "unknown part"));
	both.RunLines(nullptr, 5, '\n', PIRE_HIP_AFFIX_REST);
	what = Thrown([&] { both.HitCount(); });
	CHECK(Has(what, "pire_hip_affix_lines_gather") && Has(what, "size > 0 with null raw"));
	what = Thrown([&] { both.HitText(); });
	CHECK(Has(what, "pire_hip_affix_lines_gather") && Has(what, "size > 0 with null raw"));
	both.Run("abc", nullptr, 2).Select(PIRE_HIP_AFFIX_REST);
	what = Thrown([&] { both.Hits(); });
	CHECK(Has(what, "pire_hip_affix_run_select") && Has(what, "n > 0 with null offsets"));
	const uint64_t down[3] = {0, 3, 1};
	both.Run("abc", down, 2);
	what = Thrown([&] { both.Spans(); });
	CHECK(Has(what, "non-decreasing"));
	both.Run(none);
	CHECK(both.HitCount() == 0);
	// unknown option bits
	Runner odd(&head, &tail, 8, PIRE_HIP_AFFIX_LONGEST);
	odd.Run(none);
	what = Thrown([&] { odd.Hits(); });
	CHECK(Has(what, "pire_hip_affix_run_select") && Has(what, "unknown bits in head_opts"));

	// an absent tail: the head and the rest are there, the tail is refused
	Runner headOnly(&head, nullptr);
	headOnly.Run(none).Select(PIRE_HIP_AFFIX_HEAD);
	CHECK(headOnly.HitCount() == 0);
	headOnly.Select(PIRE_HIP_AFFIX_REST);
	CHECK(headOnly.HitCount() == 0 && headOnly.Spans().empty());
	headOnly.Select(PIRE_HIP_AFFIX_TAIL);
	what = Thrown([&] { headOnly.Hits(); });
	CHECK(Has(what, "pire_hip_affix_run_select") && Has(what, "PIRE_HIP_AFFIX_TAIL without tail_len"));
	headOnly.RunLines("", 0, '\n', PIRE_HIP_AFFIX_TAIL);
	what = Thrown([&] { headOnly.HitText(); });
	CHECK(Has(what, "pire_hip_affix_lines_gather") && Has(what, "PIRE_HIP_AFFIX_TAIL without tail_len"));
	headOnly.RunLines("", 0);
	CHECK(headOnly.LineCount() == 0 && headOnly.HitText().empty());

	// an absent head
	Runner tailOnly(nullptr, &tail);
	tailOnly.Run(none).Select(PIRE_HIP_AFFIX_TAIL);
	CHECK(tailOnly.HitCount() == 0);
	tailOnly.Select(PIRE_HIP_AFFIX_HEAD);
	what = Thrown([&] { tailOnly.Hits(); });
	CHECK(Has(what, "pire_hip_affix_run_select") && Has(what, "PIRE_HIP_AFFIX_HEAD without head_len"));
	tailOnly.RunLines("", 0, '|', PIRE_HIP_AFFIX_REST);
	CHECK(tailOnly.LineCount() == 0 && tailOnly.HitCount() == 0 && tailOnly.HitTextOffsets().size() == 1);

	// neither
	Runner neither(nullptr, nullptr);
	neither.Run(none);
	what = Thrown([&] { neither.Hits(); });
	CHECK(Has(what, "pire_hip_affix_run_select") && Has(what, "null head and null tail"));
	neither.RunLines("", 0);
	what = Thrown([&] { neither.HitText(); });
	CHECK(Has(what, "pire_hip_affix_lines_gather") && Has(what, "null head and null tail"));
}

int main()
{
	// the C ABI itself, as a caller in C++ sees it: codes and names
	uint64_t count = 77, lines = 77, bytes = 77;
	uint64_t hits[4] = {9, 9, 9, 9};
	const uint64_t offsets[4] = {0, 3, 3, 8};
	const int64_t head[3] = {1, -1, 0}, tail[3] = {0, 2, -1};
	CHECK(pire_hip_affix_select(offsets, 3, PIRE_HIP_AFFIX_REST, 0, head, tail, nullptr, nullptr, 0, nullptr, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_affix_select: null out_hit_count") == 0);
	CHECK(pire_hip_affix_select(offsets, 3, 3, 0, head, tail, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_affix_select(offsets, 3, PIRE_HIP_AFFIX_REST, 0, nullptr, nullptr, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_affix_select(offsets, 3, PIRE_HIP_AFFIX_HEAD, 0, nullptr, tail, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_affix_select(offsets, 3, PIRE_HIP_AFFIX_TAIL, 0, head, nullptr, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_affix_select(nullptr, 3, PIRE_HIP_AFFIX_REST, 0, head, tail, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_affix_select(offsets, 3, PIRE_HIP_AFFIX_REST, 0, head, tail, nullptr, nullptr, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_affix_select(offsets, uint64_t(1) << 32, PIRE_HIP_AFFIX_REST, 0, head, tail, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(count == 77);
	CHECK(pire_hip_affix_select(nullptr, 0, PIRE_HIP_AFFIX_REST, 0, nullptr, nullptr, hits, nullptr, 4, &count, nullptr) == PIRE_HIP_OK);
	CHECK(count == 0 && hits[0] == 9);
	CHECK(pire_hip_affix_lines_gather(nullptr, 1, nullptr, 1, "a\n", 2, '\n', PIRE_HIP_AFFIX_REST, 0, '\n', &lines, nullptr, nullptr, 0, &count, nullptr, 0,
	                                  nullptr, &bytes, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_affix_lines_gather: null head and null tail") == 0);
	CHECK(lines == 77 && bytes == 77);
	try {
		TestRunner();
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	if (g_fail) {
		fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(affix shim: %d checks)\n", g_checks);
	return 0;
}
