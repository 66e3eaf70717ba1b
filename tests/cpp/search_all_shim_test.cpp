// SearchBatchRunner::All() (include/pire_hip/batch_runner.hpp) as far as it is decided before a device is touched: what the
// library refuses comes back as Pire::Error with the list form's entry point in it, a batch of no strings or no bytes answers
// zeros, Rows() follows Run() alone, and Select() -- the default of every new batch -- is the first match again.  Against the
// unmodified reference headers; into oracle/_ref/bin with the libraries it links.  It needs no GPU and is run without one.
#include <cstdio>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire_hip/batch_runner.hpp>

static int g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static Pire::Fsm Parsed(const std::string& re)
{
	return Pire::Lexer(re.data(), re.data() + re.size()).Parse();
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

typedef Pire::Hip::SearchBatchRunner<Pire::Scanner> Runner;

static void TestRunner(Runner& find)
{
	const std::vector<Pire::ystring> none;
	CHECK(Has(Thrown([&] { find.All().Hits(); }), "follows Run() or RunLines()"));
	// no strings: zeros, and one row start
	find.Run(none).All();
	CHECK(find.HitCount() == 0 && find.Hits().empty() && find.Spans().empty());
	CHECK(find.Rows().size() == 1 && find.Rows()[0] == 0);
	CHECK(Has(Thrown([&] { find.LineCount(); }), "LineCount() follows RunLines()"));
	CHECK(Has(Thrown([&] { find.HitText(); }), "HitText() follows RunLines()"));
	// a new batch starts with the first match: Rows() is All()'s
	find.Run(none);
	CHECK(Has(Thrown([&] { find.Rows(); }), "Rows() follows Run() and All()"));
	find.Run(none).All().Select();
	CHECK(Has(Thrown([&] { find.Rows(); }), "Rows() follows Run() and All()"));
	// no bytes: no lines, no matches, no text -- and no rows
	find.RunLines("", 0, '\n').All();
	CHECK(find.LineCount() == 0 && find.HitCount() == 0 && find.Hits().empty() && find.Spans().empty());
	CHECK(find.HitText().empty() && find.HitTextOffsets().size() == 1 && find.HitTextOffsets()[0] == 0);
	CHECK(Has(Thrown([&] { find.Rows(); }), "Rows() follows Run() and All()"));
	find.RunLines("", 0, '|').All();
	CHECK(find.HitText('|').empty() && find.LineCount() == 0);
	// what the library refuses before it touches a device, in the name of the entry point that All() chose
	find.RunLines(nullptr, 5).All();
	std::string what = Thrown([&] { find.HitCount(); });
	CHECK(Has(what, "pire_hip_search_all_lines_gather") && Has(what, "size > 0 with null raw"));
	what = Thrown([&] { find.HitText(); });
	CHECK(Has(what, "pire_hip_search_all_lines_gather") && Has(what, "size > 0 with null raw"));
	find.RunLines(nullptr, 5);   // ... and without it, the first match's
	what = Thrown([&] { find.HitCount(); });
	CHECK(Has(what, "pire_hip_search_lines_gather") && Has(what, "size > 0 with null raw"));
	const uint64_t down[3] = {0, 3, 1};
	find.Run("abc", down, 2).All();
	what = Thrown([&] { find.Spans(); });
	CHECK(Has(what, "non-decreasing"));
	what = Thrown([&] { find.Rows(); });
	CHECK(Has(what, "non-decreasing"));
	find.Run(none).All();
	CHECK(find.HitCount() == 0);
}

int main()
{
	// the C ABI itself, as a caller in C++ sees it: codes and names
	uint64_t count = 77, lines = 77, bytes = 77, rows[4] = {9, 9, 9, 9};
	const uint64_t offsets[4] = {0, 3, 3, 8};
	CHECK(pire_hip_search_all(nullptr, nullptr, 0, "abcdefgh", 8, offsets, 3, 0, rows, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_search_all: null rev") == 0);
	CHECK(pire_hip_search_all_lines_gather(nullptr, nullptr, 0, "a\n", 2, '\n', 0, '\n', &lines, nullptr, nullptr, 0, &count, nullptr, 0, nullptr,
	                                       &bytes, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_search_all_lines_gather: null rev") == 0);
	CHECK(count == 77 && lines == 77 && bytes == 77 && rows[0] == 9 && rows[3] == 9);
	try {
		Pire::Hip::MatchFinder finder(Parsed("[0-9]+"));
		TestRunner(finder.Runner());
		// a runner over two scanners of the caller's own, and unknown option bits
		const Pire::Scanner fwd = Parsed("[0-9]+").Compile<Pire::Scanner>(), rev = Parsed("([0-9]+).*").Reverse().Compile<Pire::Scanner>();
		Runner own(rev, fwd, PIRE_HIP_SEARCH_SHORTEST);
		TestRunner(own);
		Runner odd(rev, fwd, 8);
		odd.Run(std::vector<Pire::ystring>()).All();
		std::string what = Thrown([&] { odd.Hits(); });
		CHECK(Has(what, "pire_hip_search_all") && !Has(what, "lines_gather") && Has(what, "unknown bits in opts"));
		odd.RunLines("", 0).All();
		what = Thrown([&] { odd.HitText(); });
		CHECK(Has(what, "pire_hip_search_all_lines_gather") && Has(what, "unknown bits in opts"));
		Pire::Hip::MatchFinder marked(Parsed("[a-z]+$"), PIRE_HIP_SEARCH_THROUGH_END);
		marked.Runner().RunLines("", 0).All();
		CHECK(marked.Runner().HitCount() == 0);
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	if (g_fail) {
		fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(search_all shim: %d checks)\n", g_checks);
	return 0;
}
