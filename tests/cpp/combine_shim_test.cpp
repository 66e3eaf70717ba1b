// LineQuery and Truth (include/pire_hip/batch_runner.hpp) as far as they are decided before a device is touched: what Truth::*
// builds, what the library refuses comes back as Pire::Error with the entry point's name in it, a buffer of no bytes answers
// zeros, and the accessors follow RunLines().  Fsms built as easy.h builds them, against the unmodified reference headers; into
// oracle/_ref/bin with the libraries it links.  It needs no GPU and is run without one.
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

typedef std::vector<uint64_t> U64s;
using Pire::Hip::Truth;

static bool One(unsigned m) { return m == 1 || m == 2 || m == 4; }

static void TestTruth()
{
	CHECK(Truth::All(1) == 0x2 && Truth::All(2) == 0x8 && Truth::All(3) == 0x80 && Truth::All(6) == uint64_t(1) << 63);
	CHECK(Truth::Any(1) == 0x2 && Truth::Any(2) == 0xE && Truth::Any(3) == 0xFE && Truth::Any(6) == ~uint64_t(1));
	CHECK(Truth::Of(2, [](unsigned m) { return m == 1; }) == 0x2);            // the first and not the second
	CHECK(Truth::Of(1, [](unsigned m) { return m == 0; }) == 0x1);            // the complement
	CHECK(Truth::Of(3, One) == 0x16);                                         // exactly one of three
	CHECK(Truth::Of(6, [](unsigned) { return true; }) == ~uint64_t(0));
	CHECK(Truth::Of(4, [](unsigned) { return false; }) == 0);
	CHECK(Has(Thrown([] { Truth::All(0); }), "1 .. 6 terms") && Has(Thrown([] { Truth::Any(7); }), "1 .. 6 terms"));
}

// a query with a buffer of no bytes behind RunLines(): zeros from every accessor
static void CheckEmpty(Pire::Hip::LineQuery& q)
{
	CHECK(q.LineCount() == 0 && q.HitCount() == 0);
	CHECK(q.Hits().empty() && q.HitSpans().empty() && q.HitMembers().empty());
	CHECK(q.TermCounts() == U64s(q.Terms(), 0));
	CHECK(q.HitText().empty() && q.HitTextOffsets() == U64s(1, 0));
	CHECK(q.HitText('|').empty());
}

static void TestLineQuery()
{
	const Pire::Scanner fast = Surrounded("a.{3}b").Compile<Pire::Scanner>();
	const Pire::Scanner other = Surrounded("xyz").Compile<Pire::Scanner>();
	const Pire::SlowScanner slow = Surrounded("a.{20}$").Compile<Pire::SlowScanner>();
	Pire::Hip::LineQuery q;
	// the accessors follow RunLines()
	CHECK(Has(Thrown([&] { q.Hits(); }), "Hits() follows RunLines()"));
	q.Add(fast);
	CHECK(Has(Thrown([&] { q.Hits(); }), "Hits() follows RunLines()"));
	CHECK(Has(Thrown([&] { q.HitSpans(); }), "HitSpans() follows RunLines()"));
	CHECK(Has(Thrown([&] { q.HitMembers(); }), "HitMembers() follows RunLines()"));
	CHECK(Has(Thrown([&] { q.TermCounts(); }), "TermCounts() follows RunLines()"));
	CHECK(Has(Thrown([&] { q.HitText(); }), "HitText() follows RunLines()"));
	CHECK(Has(Thrown([&] { q.HitCount(); }), "HitCount() follows RunLines()"));
	// no bytes: zeros, whatever the terms and the table
	q.RunLines("", 0);
	CheckEmpty(q);
	q.AddSlow(slow, true).AddField(other, 2).AddField(other, 0, ',', true);
	CHECK(q.Terms() == 4);
	q.RunLines("", 0);
	CheckEmpty(q);
	q.Where(Truth::Of(4, [](unsigned m) { return m == 0; })).RunLines(nullptr, 0, '|');
	CheckEmpty(q);
	// what the library refuses before it touches a device
	q.RunLines(nullptr, 5);
	std::string what = Thrown([&] { q.Hits(); });
	CHECK(Has(what, "pire_hip_lines_combine_select: ") && Has(what, "size > 0 with null raw"));
	what = Thrown([&] { q.HitText(); });
	CHECK(Has(what, "pire_hip_lines_combine_gather: ") && Has(what, "size > 0 with null raw"));
	q.RunLines("a,b\nc", 5, ',');                      // the delimiter is the separator of term 3
	what = Thrown([&] { q.HitCount(); });
	CHECK(Has(what, "pire_hip_lines_combine_select: ") && Has(what, "term 3: sep == delim"));
	Pire::Hip::LineQuery none;
	none.RunLines("ab\n", 3);
	what = Thrown([&] { none.Hits(); });
	CHECK(Has(what, "pire_hip_lines_combine_select: ") && (Has(what, "null terms") || Has(what, "k_terms == 0")));
	none.RunLines("", 0);                              // (refused on an empty buffer too: the terms are looked at first)
	CHECK(!Thrown([&] { none.HitText(); }).empty());
	Pire::Hip::LineQuery seven;
	for (int k = 0; k < 7; ++k)
		seven.Add(other);
	seven.RunLines("ab\n", 3);
	what = Thrown([&] { seven.Hits(); });
	CHECK(Has(what, "pire_hip_lines_combine_select: ") && Has(what, "more than 6 terms"));
	what = Thrown([&] { seven.HitText(); });
	CHECK(Has(what, "pire_hip_lines_combine_gather: ") && Has(what, "more than 6 terms"));
}

int main()
{
	// the C ABI itself, as a caller in C++ sees it: codes and names
	uint64_t count = 77, lines = 77, out[4] = {9, 9, 9, 9}, termCounts[2] = {9, 9};
	uint8_t members[4] = {9, 9, 9, 9};
	const uint64_t a[3] = {1, 4, 6}, b[2] = {2, 4}, unsorted[3] = {4, 1, 6};
	const uint64_t* two[2] = {a, b};
	const uint64_t* bad[2] = {a, unsorted};
	const uint64_t* holed[2] = {a, nullptr};
	const uint64_t caps[2] = {3, 2}, caps3[2] = {3, 3}, huge[2] = {3, uint64_t(1) << 32};
	const uint64_t* seven[7] = {a, a, a, a, a, a, a};
	const uint64_t caps7[7] = {3, 3, 3, 3, 3, 3, 3};
	CHECK(pire_hip_combine(two, nullptr, caps, 0, 8, 2, 0, out, members, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_combine: k_lists == 0") == 0);
	CHECK(pire_hip_combine(seven, nullptr, caps7, 7, 8, 2, 0, out, members, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_combine: more than 6 lists") == 0);
	CHECK(pire_hip_combine(nullptr, nullptr, caps, 2, 8, 2, 0, out, members, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_combine: null lists") == 0);
	CHECK(pire_hip_combine(two, nullptr, nullptr, 2, 8, 2, 0, out, members, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_combine: null list_caps") == 0);
	CHECK(pire_hip_combine(holed, nullptr, caps, 2, 8, 2, 0, out, members, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_combine: list_caps[1] > 0 with null lists[1]") == 0);
	CHECK(pire_hip_combine(two, nullptr, caps, 2, 8, 2, 0, out, members, 4, nullptr, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_combine: null out_hit_count") == 0);
	CHECK(pire_hip_combine(two, nullptr, caps, 2, 8, 2, 0, nullptr, nullptr, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_combine: hit_cap > 0 with null out_hits") == 0);
	CHECK(pire_hip_combine(two, nullptr, caps, 2, 8, 2, 0, nullptr, members, 0, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_combine: out_hit_members without out_hits") == 0);
	CHECK(pire_hip_combine(two, nullptr, caps, 2, uint64_t(1) << 32, 2, 0, out, members, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_combine(two, nullptr, huge, 2, 8, 2, 0, out, members, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	// host pointers: the lists are looked at before anything is written
	CHECK(pire_hip_combine(bad, nullptr, caps3, 2, 8, 2, 0, out, members, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_combine: list 1 must be strictly ascending") == 0);
	CHECK(pire_hip_combine(two, nullptr, caps, 2, 6, 2, 0, out, members, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_combine: list 0 names a line out of range") == 0);
	CHECK(count == 77 && out[0] == 9 && members[0] == 9);
	// no lines: a count of 0, no device is touched
	const uint64_t noCaps[2] = {0, 0};
	CHECK(pire_hip_combine(holed, nullptr, noCaps, 2, 0, 1, 0, out, members, 4, &count, nullptr) == PIRE_HIP_OK);
	CHECK(count == 0 && out[0] == 9 && members[0] == 9);
	// the lines forms
	count = 77;
	pire_hip_line_term neither[2] = {};
	neither[0].column = neither[1].column = PIRE_HIP_TERM_LINE;
	CHECK(pire_hip_lines_combine_select(nullptr, 2, 8, "a\n", 2, '\n', 0, &lines, nullptr, nullptr, nullptr, 0, &count, termCounts, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_lines_combine_select: null terms") == 0);
	CHECK(pire_hip_lines_combine_select(neither, 2, 8, "a\n", 2, '\n', 0, &lines, nullptr, nullptr, nullptr, 0, &count, termCounts, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_lines_combine_select: term 0: neither table nor slow_table") == 0);
	CHECK(pire_hip_lines_combine_gather(neither, 2, 8, "a\n", 2, '\n', 0, &lines, nullptr, nullptr, nullptr, 0, &count, termCounts, '\n', nullptr, 0,
	                                    nullptr, &lines, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_lines_combine_gather: term 0: neither table nor slow_table") == 0);
	CHECK(lines == 77 && count == 77 && termCounts[0] == 9);
	try {
		TestTruth();
		TestLineQuery();
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	if (g_fail) {
		fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(combine shim: %d checks)\n", g_checks);
	return 0;
}
