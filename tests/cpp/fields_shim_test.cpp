// BatchRunner::RunLinesField of include/pire_hip/batch_runner.hpp -- Hits(), HitSpans(), HitText(), HitTextOffsets() -- against
// the host loop it replaces, in the reference's own vocabulary: std::getline cuts the lines, the column is cut by hand, and
// Pire::Runner(sc).Begin().Run(field).End() of the unmodified reference says whether the line is selected.  Built like
// shim_test.cpp, into oracle/_ref/bin with the libraries it links.
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire_hip/batch_runner.hpp>

static int g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static Pire::Scanner Compile(const char* re)
{
	Pire::Fsm fsm = Pire::Lexer(re, re + strlen(re)).Parse();
	return fsm.Compile<Pire::Scanner>();   // (not surrounded: ^ and $ are the pattern's own, and they anchor to the column)
}

// column `field` of a line: the run between separators number field - 1 and field, to the end of the line with `rest`; empty
// where the line has too few
static std::string Column(const std::string& line, size_t field, char sep, bool rest)
{
	size_t begin = 0;
	for (size_t k = 0; k < field; ++k) {
		const size_t at = line.find(sep, begin);
		if (at == std::string::npos)
			return std::string();
		begin = at + 1;
	}
	const size_t end = rest ? std::string::npos : line.find(sep, begin);
	return line.substr(begin, end == std::string::npos ? std::string::npos : end - begin);
}

struct Want {
	std::vector<uint64_t> hits, spans;
	std::string text;
	std::vector<uint64_t> textOffsets;
	uint64_t lines;
};

// the host loop
static Want HostLoop(const Pire::Scanner& sc, const std::string& raw, size_t field, char sep, bool rest)
{
	Want w;
	w.lines = 0;
	w.textOffsets.push_back(0);
	std::istringstream in(raw);
	std::string line;
	uint64_t at = 0;
	while (std::getline(in, line)) {
		const std::string col = Column(line, field, sep, rest);
		if (Pire::Runner(sc).Begin().Run(col.data(), col.size()).End()) {
			w.hits.push_back(w.lines);
			w.spans.push_back(at);
			w.spans.push_back(at + line.size());
			w.text += line;
			w.text += '\n';
			w.textOffsets.push_back(w.text.size());
		}
		at += line.size() + 1;
		++w.lines;
	}
	return w;
}

static void Compare(const Pire::Scanner& sc, const std::string& raw, size_t field, char sep, bool rest)
{
	const Want want = HostLoop(sc, raw, field, sep, rest);
	Pire::Hip::Table<Pire::Scanner> table(sc);
	{
		Pire::Hip::BatchRunner<Pire::Scanner> gpu(table);
		gpu.Begin().RunLinesField(raw.data(), raw.size(), uint32_t(field), sep, '\n', rest).End();
		CHECK(gpu.Hits() == want.hits);
		CHECK(gpu.HitSpans() == want.spans);
		CHECK(gpu.HitCount() == want.hits.size());
		CHECK(gpu.LineCount() == want.lines);
		CHECK(gpu.HitText() == want.text);
		CHECK(gpu.HitTextOffsets() == want.textOffsets);
		for (size_t k = 0; k < want.hits.size() && k < gpu.HitSpans().size() / 2; ++k)
			CHECK(raw.compare(size_t(gpu.HitSpans()[2 * k]), size_t(gpu.HitSpans()[2 * k + 1] - gpu.HitSpans()[2 * k]),
			                  want.text, size_t(want.textOffsets[k]), size_t(want.textOffsets[k + 1] - want.textOffsets[k] - 1)) == 0);
		// the accessors RunLines() refuses stay refused, and there is no per-regexp form of this call
		bool threw = false;
		try {
			gpu.States();
		} catch (const Pire::Error&) {
			threw = true;
		}
		CHECK(threw);
		threw = false;
		try {
			gpu.Route().RouteCount(0);
		} catch (const Pire::Error&) {
			threw = true;
		}
		CHECK(threw);
	}
	{
		// the text first, no delimiter behind the lines; then the lists, from a runner that has not scanned yet
		Pire::Hip::BatchRunner<Pire::Scanner> gpu(table);
		gpu.Begin().RunLinesField(raw.data(), raw.size(), uint32_t(field), sep, '\n', rest).End();
		std::string bare;
		for (size_t k = 0; k + 1 < want.textOffsets.size(); ++k)
			bare.append(want.text, size_t(want.textOffsets[k]), size_t(want.textOffsets[k + 1] - want.textOffsets[k] - 1));
		CHECK(gpu.HitText('\0').size() == bare.size() + want.hits.size());
		CHECK(gpu.Hits() == want.hits);
		// ... and RunLines() on the same runner afterwards scans whole lines again
		gpu.Begin().RunLines(raw.data(), raw.size()).End();
		const Want whole = HostLoop(sc, raw, 0, '\n', true);
		CHECK(gpu.Hits() == whole.hits);
		CHECK(gpu.HitText() == whole.text);
	}
}

int main()
{
	const char* words[] = {"alpha", "beta", "GET /index.html", "http://example.com/a?b=c", "", "x", "404", "needle", "a needle here",
	                       "needles", "NEEDLE", "-"};
	const size_t nwords = sizeof(words) / sizeof(words[0]);
	// a few hundred lines of 0 to 5 columns; every third line's last column holds the separator's neighbour, an empty column
	std::string raw;
	uint32_t x = 12345;
	for (size_t i = 0; i < 400; ++i) {
		const size_t cols = (x = x * 1664525u + 1013904223u) >> 29;   // 0..7
		for (size_t c = 0; c < cols % 6; ++c) {
			if (c)
				raw.push_back('\t');
			raw += words[((x = x * 1664525u + 1013904223u) >> 16) % nwords];
		}
		if (i % 3 == 0)
			raw.push_back('\t');
		raw.push_back('\n');
	}
	std::string open = raw;
	open += "k\tv\tneedle";   // no delimiter behind the last line

	const Pire::Scanner needle = Compile("needle"), anchored = Compile("^needle$"), any = Compile("^.*$"), empty = Compile("^$");
	for (size_t field = 0; field < 4; ++field) {
		Compare(needle, raw, field, '\t', false);
		Compare(anchored, raw, field, '\t', false);
		Compare(anchored, open, field, '\t', field == 2);
	}
	Compare(needle, raw, 1, '\t', true);
	Compare(empty, raw, 2, '\t', false);
	Compare(needle, open, 40, '\t', false);
	Compare(needle, raw, 1, ' ', false);
	// more hits than the first call has room for (size / 64 + 1024): every line of a buffer of short lines
	std::string many;
	for (size_t i = 0; i < 3000; ++i)
		many += i % 2 ? "a\tb\n" : "\n";
	CHECK(many.size() / 64 + 1024 < 3000);
	Compare(any, many, 1, '\t', false);
	Compare(empty, many, 1, '\t', false);
	Compare(needle, std::string(), 0, '\t', false);
	Compare(empty, std::string("\n\n\n"), 3, '\t', false);

	if (g_fail) {
		fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(fields shim: %d checks)\n", g_checks);
	return 0;
}
