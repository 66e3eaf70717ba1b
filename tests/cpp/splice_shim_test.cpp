// Substitution (include/pire_hip/batch_runner.hpp) as far as it is decided before a device is touched: what the library
// refuses comes back as Pire::Error with pire_hip_search_lines_splice in it, a buffer of no bytes answers zeros whatever the
// pieces are, an accessor without a buffer throws, and the pieces can be changed between two fetches.  Against the unmodified
// reference headers; into oracle/_ref/bin with the libraries it links.  It needs no GPU and is run without one.
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

static void TestSubstitution(Pire::Hip::Substitution& sub)
{
	// no bytes: no lines, no matches, no text -- under every piece and both forms of the search
	sub.RunLines("", 0);
	CHECK(sub.Text().empty() && sub.Bytes() == 0 && sub.MatchCount() == 0 && sub.LineCount() == 0);
	sub.With("#").RunLines("", 0, '|');
	CHECK(sub.Text().empty() && sub.Bytes() == 0 && sub.MatchCount() == 0 && sub.LineCount() == 0);
	sub.Wrap("<b>", "</b>").FirstOnly().RunLines("", 0);
	CHECK(sub.Text().empty() && sub.LineCount() == 0);
	sub.Delete().FirstOnly(false);
	CHECK(sub.Bytes() == 0);
	// what the library refuses before it touches a device, in the entry point's name
	sub.RunLines(nullptr, 5);
	std::string what = Thrown([&] { sub.Text(); });
	CHECK(Has(what, "pire_hip_search_lines_splice") && Has(what, "size > 0 with null raw"));
	what = Thrown([&] { sub.MatchCount(); });   // (a refused call is not remembered as a result)
	CHECK(Has(what, "pire_hip_search_lines_splice") && Has(what, "size > 0 with null raw"));
	sub.With(std::string(257, 'x')).RunLines("", 0);
	what = Thrown([&] { sub.Bytes(); });
	CHECK(Has(what, "pire_hip_search_lines_splice") && Has(what, "head_len > 256"));
	sub.Wrap("(", std::string(300, ')'));
	what = Thrown([&] { sub.LineCount(); });
	CHECK(Has(what, "pire_hip_search_lines_splice") && Has(what, "tail_len > 256"));
	sub.With(std::string(256, 'x'));   // the longest piece there is: fine
	CHECK(sub.Bytes() == 0 && sub.Text().empty());
	sub.RunLines("", 0, '\0').Delete();
	CHECK(sub.LineCount() == 0);
}

int main()
{
	// the C ABI itself, as a caller in C++ sees it: codes and names
	uint64_t count = 77, lines = 77, bytes = 77, pos[2] = {9, 9};
	const uint64_t spans[4] = {1, 2, 3, 5};
	char out[16] = {0};
	CHECK(pire_hip_splice("a1b22c", 6, spans, nullptr, 2, "#", 1, nullptr, 0, 4, nullptr, 0, 0, out, 16, pos, nullptr, &bytes, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_splice: unknown bits in mode") == 0);
	const uint64_t back[4] = {3, 5, 1, 2};
	CHECK(pire_hip_splice("a1b22c", 6, back, nullptr, 2, "#", 1, nullptr, 0, 0, nullptr, 0, 0, out, 16, pos, nullptr, &bytes, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_splice: spans must ascend") == 0);
	CHECK(pire_hip_search_lines_splice(nullptr, nullptr, 0, "a\n", 2, '\n', 0, "#", 1, nullptr, 0, 0, &lines, nullptr, nullptr, 4, &count, out, 16, &bytes,
	                                   nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_search_lines_splice: null rev") == 0);
	CHECK(count == 77 && lines == 77 && bytes == 77 && pos[0] == 9 && out[0] == 0);
	try {
		Pire::Hip::MatchFinder finder(Parsed("[0-9]+"));
		CHECK(finder.Opts() == 0);
		Pire::Hip::Substitution sub(finder);
		CHECK(Has(Thrown([&] { sub.Text(); }), "Text() follows RunLines()"));
		TestSubstitution(sub);
		Pire::Hip::MatchFinder marked(Parsed("[a-z]+$"), PIRE_HIP_SEARCH_THROUGH_END | PIRE_HIP_SEARCH_SHORTEST);
		CHECK(marked.Opts() == (PIRE_HIP_SEARCH_THROUGH_END | PIRE_HIP_SEARCH_SHORTEST));
		Pire::Hip::Substitution end(marked);
		TestSubstitution(end);
		// unknown option bits of the finder are the search's to refuse, in this entry point's name
		Pire::Hip::MatchFinder odd(Parsed("[0-9]+"), 8);
		Pire::Hip::Substitution oddSub(odd);
		oddSub.With("#").RunLines("", 0);
		const std::string what = Thrown([&] { oddSub.Text(); });
		CHECK(Has(what, "pire_hip_search_lines_splice") && Has(what, "unknown bits in opts"));
		// the finder's own runner is untouched by a Substitution over it
		finder.Runner().RunLines("", 0);
		CHECK(finder.Runner().HitCount() == 0 && finder.Runner().LineCount() == 0);
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	if (g_fail) {
		fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(splice shim: %d checks)\n", g_checks);
	return 0;
}
