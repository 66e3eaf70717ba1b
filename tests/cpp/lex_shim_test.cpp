// TokenFinder and LexBatchRunner (include/pire_hip/batch_runner.hpp) as far as they are decided before a device is touched:
// TokenFinder builds both scanners of pire_hip_lex from the regexps' Fsms -- their Save() forms are written out for the caller to
// hold against the fixtures the reference wrote (tests/golden/lex) --, what the library refuses comes back as Pire::Error with
// the entry point in it, a batch of no strings or no bytes answers zeros, and the lists follow a Run().  Against the unmodified
// reference headers; into oracle/_ref/bin with the libraries it links.  It needs no GPU and is run without one.
//   lex_shim_test SETS OUTDIR     SETS: lines of  name <tab> pattern <tab> pattern ...;  OUTDIR/<name>.n.blob, OUTDIR/<name>.nr.blob
#include <cstdio>
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

typedef Pire::Hip::LexBatchRunner Runner;

static void TestRunner(Runner& lex, size_t regexps)
{
	const std::vector<Pire::ystring> none;
	// nothing before a Run()
	CHECK(Has(Thrown([&] { lex.Labels(); }), "Labels() follows Run() or RunLines()"));
	CHECK(Has(Thrown([&] { lex.Masks(); }), "Masks() follows Run() or RunLines()"));
	CHECK(Has(Thrown([&] { lex.Rows(); }), "Rows() follows Run()"));
	CHECK(Has(Thrown([&] { lex.Tokens().Hits(); }), "Hits() follows Run() or RunLines()"));
	for (int tokens = 0; tokens < 2; ++tokens) {
		// no strings: zeros, one row start, R + 1 label counts
		lex.Run(none).Tokens(tokens != 0);
		CHECK(lex.HitCount() == 0 && lex.Hits().empty() && lex.Spans().empty() && lex.Masks().empty() && lex.Labels().empty());
		CHECK(lex.Rows().size() == 1 && lex.Rows()[0] == 0);
		CHECK(lex.LabelCounts().size() == regexps + 1 && lex.LabelCounts()[0] == 0 && lex.LabelCounts()[regexps] == 0);
		CHECK(Has(Thrown([&] { lex.LineCount(); }), "LineCount() follows RunLines()"));
		CHECK(Has(Thrown([&] { lex.HitText(); }), "HitText() follows RunLines()"));
		// no bytes: no lines, no entries, no text -- and no rows
		lex.RunLines("", 0, '\n').Tokens(tokens != 0);
		CHECK(lex.LineCount() == 0 && lex.HitCount() == 0 && lex.Hits().empty() && lex.Spans().empty() && lex.Masks().empty());
		CHECK(lex.LabelCounts().size() == regexps + 1 && lex.LabelCounts()[regexps] == 0);
		CHECK(lex.HitText().empty() && lex.HitTextOffsets().size() == 1 && lex.HitTextOffsets()[0] == 0);
		CHECK(Has(Thrown([&] { lex.Rows(); }), "Rows() follows Run()"));
		// what the library refuses before it touches a device, in the name of the entry point
		lex.RunLines(nullptr, 5).Tokens(tokens != 0);
		std::string what = Thrown([&] { lex.HitCount(); });
		CHECK(Has(what, "pire_hip_lex_lines_gather") && Has(what, "size > 0 with null raw"));
		what = Thrown([&] { lex.HitText(); });
		CHECK(Has(what, "pire_hip_lex_lines_gather") && Has(what, "size > 0 with null raw"));
		const uint64_t down[3] = {0, 3, 1};
		lex.Run("abc", down, 2).Tokens(tokens != 0);
		what = Thrown([&] { lex.Masks(); });
		CHECK(Has(what, "non-decreasing"));
		what = Thrown([&] { lex.Rows(); });
		CHECK(Has(what, "non-decreasing"));
	}
	lex.Run(none);
	CHECK(lex.HitCount() == 0);
}

int main(int argc, char** argv)
{
	if (argc != 3) {
		fprintf(stderr, "usage: lex_shim_test SETS OUTDIR\n");
		return 2;
	}
	// the C ABI itself, as a caller in C++ sees it: codes and names
	uint64_t count = 77, lines = 77, bytes = 77, rows[4] = {9, 9, 9, 9};
	const uint64_t offsets[4] = {0, 3, 3, 8};
	CHECK(pire_hip_lex(nullptr, nullptr, 0, "abcdefgh", 8, offsets, 3, 0, rows, nullptr, nullptr, nullptr, 0, &count, nullptr, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_lex: null fwd") == 0);
	CHECK(pire_hip_lex_lines_gather(nullptr, nullptr, PIRE_HIP_LEX_TOKENS, "a\n", 2, '\n', 0, '\n', &lines, nullptr, nullptr, nullptr, 0, &count, nullptr,
	                                nullptr, 0, nullptr, &bytes, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_lex_lines_gather: null fwd") == 0);
	CHECK(count == 77 && lines == 77 && bytes == 77 && rows[0] == 9 && rows[3] == 9);
	CHECK(PIRE_HIP_LEX_SHORTEST == 1u && PIRE_HIP_LEX_THROUGH_BEGIN == 2u && PIRE_HIP_LEX_THROUGH_END == 4u && PIRE_HIP_LEX_TOKENS == 8u);
	try {
		// both scanners of every set from the regexps' Fsms: written out, the caller compares them with what the reference wrote
		std::ifstream in(argv[1]);
		std::string line;
		int sets = 0;
		while (std::getline(in, line)) {
			std::vector<std::string> fields;
			for (size_t at = 0;;) {
				const size_t tab = line.find('\t', at);
				fields.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
				if (tab == std::string::npos)
					break;
				at = tab + 1;
			}
			if (fields.size() < 2)
				continue;
			std::vector<Pire::Fsm> rules;
			std::string unionRe;
			for (size_t i = 1; i < fields.size(); ++i) {
				rules.push_back(Parsed(fields[i]));
				unionRe += (i > 1 ? "|(" : "(") + fields[i] + ")";
			}
			Pire::Hip::TokenFinder finder(rules);
			const std::string fwd = Pire::Hip::SavedBlob(finder.Forward()), rev = Pire::Hip::SavedBlob(finder.ReversedTail());
			std::ofstream((std::string(argv[2]) + "/" + fields[0] + ".n.blob").c_str(), std::ios::binary).write(fwd.data(), fwd.size());
			std::ofstream((std::string(argv[2]) + "/" + fields[0] + ".nr.blob").c_str(), std::ios::binary).write(rev.data(), rev.size());
			CHECK(finder.Forward().RegexpsCount() == rules.size());
			// ... and the reversed one is what the documented recipe gives
			CHECK(rev == Pire::Hip::SavedBlob(Parsed("(" + unionRe + ").*").Reverse().Compile<Pire::Scanner>()));
			if (sets == 0)
				TestRunner(finder.Runner(), rules.size());
			++sets;
		}
		CHECK(sets > 0);
		// what TokenFinder itself refuses
		CHECK(Has(Thrown([&] { Pire::Hip::TokenFinder none((std::vector<Pire::Fsm>())); }), "1 to 64 regexps"));
		std::vector<Pire::Fsm> many;
		for (int i = 0; i < 65; ++i)
			many.push_back(Parsed("k" + std::to_string(i)));
		CHECK(Has(Thrown([&] { Pire::Hip::TokenFinder big(many); }), "1 to 64 regexps"));
		// a runner over two scanners of the caller's own, and unknown option bits
		const Pire::Scanner fwd = Pire::Scanner::Glue(Parsed("[0-9]+").Compile<Pire::Scanner>(), Parsed("[a-z]+").Compile<Pire::Scanner>());
		const Pire::Scanner rev = Parsed("(([0-9]+)|([a-z]+)).*").Reverse().Compile<Pire::Scanner>();
		Runner own(rev, fwd, PIRE_HIP_LEX_SHORTEST);
		TestRunner(own, 2);
		Runner odd(rev, fwd, 16);
		odd.Run(std::vector<Pire::ystring>());
		std::string what = Thrown([&] { odd.Hits(); });
		CHECK(Has(what, "pire_hip_lex") && !Has(what, "lines_gather") && Has(what, "unknown bits in opts"));
		odd.RunLines("", 0).Tokens();
		what = Thrown([&] { odd.HitText(); });
		CHECK(Has(what, "pire_hip_lex_lines_gather") && Has(what, "unknown bits in opts"));
		// more than 64 regexps in a scanner of the caller's own: refused by the library
		Pire::Scanner wide = many[0].Compile<Pire::Scanner>();
		for (size_t i = 1; i < many.size(); ++i)
			wide = Pire::Scanner::Glue(wide, many[i].Compile<Pire::Scanner>());
		Runner tooMany(rev, wide);
		tooMany.Run(std::vector<Pire::ystring>()).Tokens();
		what = Thrown([&] { tooMany.Masks(); });
		CHECK(Has(what, "pire_hip_lex") && Has(what, "65 regexps"));
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	if (g_fail) {
		fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(lex shim: %d checks)\n", g_checks);
	return 0;
}
