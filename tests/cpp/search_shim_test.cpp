// SearchBatchRunner and MatchFinder (include/pire_hip/batch_runner.hpp) as far as it is decided before a device is touched:
// MatchFinder builds both scanners of a search from one Fsm -- their Save() forms are written out for the caller to hold
// against the fixtures the reference wrote (tests/golden/search) --, what the library refuses comes back as Pire::Error with
// the entry point's name in it, and a batch of no strings or no bytes answers zeros.  Against the unmodified reference
// headers; into oracle/_ref/bin with the libraries it links.  It needs no GPU and is run without one.
//
//   search_shim_test PATTERNS OUTDIR     PATTERNS: lines of  name <tab> pattern;  OUTDIR/<name>.n.blob, OUTDIR/<name>.nr.blob
#include <cstdio>
#include <cstring>
#include <fstream>
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
	CHECK(Has(Thrown([&] { find.Hits(); }), "follows Run() or RunLines()"));
	// no strings: zeros
	find.Run(none).Select();
	CHECK(find.HitCount() == 0 && find.Hits().empty() && find.Spans().empty());
	CHECK(Has(Thrown([&] { find.LineCount(); }), "LineCount() follows RunLines()"));
	CHECK(Has(Thrown([&] { find.HitText(); }), "HitText() follows RunLines()"));
	// no bytes: no lines, no hits, no text
	find.RunLines("", 0, '\n');
	CHECK(find.LineCount() == 0 && find.HitCount() == 0 && find.Hits().empty() && find.Spans().empty());
	CHECK(find.HitText().empty() && find.HitTextOffsets().size() == 1 && find.HitTextOffsets()[0] == 0);
	find.RunLines("", 0, '|');
	CHECK(find.HitText('|').empty() && find.LineCount() == 0);
	// what the library refuses before it touches a device
	find.RunLines(nullptr, 5);
	std::string what = Thrown([&] { find.HitCount(); });
	CHECK(Has(what, "pire_hip_search_lines_gather") && Has(what, "size > 0 with null raw"));
	what = Thrown([&] { find.HitText(); });
	CHECK(Has(what, "pire_hip_search_lines_gather") && Has(what, "size > 0 with null raw"));
	find.Run("abc", nullptr, 2);
	what = Thrown([&] { find.Hits(); });
	CHECK(Has(what, "pire_hip_search_run_select") && Has(what, "n > 0 with null text or offsets"));
	const uint64_t down[3] = {0, 3, 1};
	find.Run("abc", down, 2);
	what = Thrown([&] { find.Spans(); });
	CHECK(Has(what, "non-decreasing"));
	find.Run(none);
	CHECK(find.HitCount() == 0);
}

int main(int argc, char** argv)
{
	if (argc != 3) {
		fprintf(stderr, "usage: search_shim_test PATTERNS OUTDIR\n");
		return 2;
	}
	// the C ABI itself, as a caller in C++ sees it: codes and names
	uint64_t count = 77, lines = 77, bytes = 77;
	int64_t begin[3] = {9, 9, 9}, end[3] = {9, 9, 9};
	const uint64_t offsets[4] = {0, 3, 3, 8};
	CHECK(pire_hip_search(nullptr, nullptr, 0, "abcdefgh", offsets, 3, 0, begin, end, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_search: null rev") == 0);
	CHECK(pire_hip_search_run_select(nullptr, nullptr, 0, "abcdefgh", offsets, 3, 0, begin, end, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_search_run_select: null rev") == 0);
	CHECK(pire_hip_search_lines_gather(nullptr, nullptr, 0, "a\n", 2, '\n', 0, '\n', &lines, nullptr, nullptr, 0, &count, nullptr, 0, nullptr, &bytes,
	                                   nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_search_lines_gather: null rev") == 0);
	CHECK(count == 77 && lines == 77 && bytes == 77 && begin[0] == 9 && end[2] == 9);
	CHECK(PIRE_HIP_SEARCH_SHORTEST == 1u && PIRE_HIP_SEARCH_THROUGH_BEGIN == 2u && PIRE_HIP_SEARCH_THROUGH_END == 4u);
	try {
		// both scanners of every pair from one Fsm: written out, the caller compares them with what the reference wrote
		std::ifstream in(argv[1]);
		std::string line;
		int pairs = 0;
		while (std::getline(in, line)) {
			const size_t tab = line.find('\t');
			if (tab == std::string::npos)
				continue;
			const std::string name = line.substr(0, tab), pattern = line.substr(tab + 1);
			Pire::Hip::MatchFinder finder(Parsed(pattern));
			const std::string fwd = Pire::Hip::SavedBlob(finder.Forward()), rev = Pire::Hip::SavedBlob(finder.ReversedTail());
			std::ofstream((std::string(argv[2]) + "/" + name + ".n.blob").c_str(), std::ios::binary).write(fwd.data(), fwd.size());
			std::ofstream((std::string(argv[2]) + "/" + name + ".nr.blob").c_str(), std::ios::binary).write(rev.data(), rev.size());
			// ... and they are what the two documented recipes give
			CHECK(fwd == Pire::Hip::SavedBlob(Parsed(pattern).Compile<Pire::Scanner>()));
			CHECK(rev == Pire::Hip::SavedBlob(Parsed("(" + pattern + ").*").Reverse().Compile<Pire::Scanner>()));
			if (pairs == 0)
				TestRunner(finder.Runner());
			++pairs;
		}
		CHECK(pairs > 0);
		// a runner over two scanners of the caller's own, and unknown option bits
		const Pire::Scanner fwd = Parsed("[0-9]+").Compile<Pire::Scanner>(), rev = Parsed("([0-9]+).*").Reverse().Compile<Pire::Scanner>();
		Runner own(rev, fwd, PIRE_HIP_SEARCH_SHORTEST);
		TestRunner(own);
		Runner odd(rev, fwd, 8);
		odd.Run(std::vector<Pire::ystring>());
		std::string what = Thrown([&] { odd.Hits(); });
		CHECK(Has(what, "pire_hip_search_run_select") && Has(what, "unknown bits in opts"));
		odd.RunLines("", 0);
		what = Thrown([&] { odd.HitText(); });
		CHECK(Has(what, "pire_hip_search_lines_gather") && Has(what, "unknown bits in opts"));
		Pire::Hip::MatchFinder marked(Parsed("[a-z]+$"), PIRE_HIP_SEARCH_THROUGH_END);
		marked.Runner().RunLines("", 0);
		CHECK(marked.Runner().HitCount() == 0);
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	if (g_fail) {
		fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(search shim: %d checks)\n", g_checks);
	return 0;
}
