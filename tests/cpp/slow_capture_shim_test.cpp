// SlowCaptureBatchRunner (include/pire_hip/batch_runner.hpp) as far as it is decided before a device is touched: construction
// from a Pire::SlowCapturingScanner compiled as the reference's own capture test compiles one, what the library refuses comes
// back as Pire::Error with the entry point's name in it, batches of no strings and buffers of no bytes answer zeros, and the
// accessors follow Run() / RunLines().  Against the unmodified reference headers; into oracle/_ref/bin with the libraries it
// links.  It needs no GPU and is run without one.
#include <cstdio>
#include <cstring>
#include <iterator>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire/extra.h>
#include <pire_hip/batch_runner.hpp>

static int g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

// capture_ut.cpp:54-65
static Pire::SlowCapturingScanner SlowCompile(const char* regexp, size_t index)
{
	const Pire::Encoding& encoding = Pire::Encodings::Utf8();
	Pire::Lexer lexer;
	lexer.AddFeature(Pire::Features::Capture(index));
	lexer.SetEncoding(encoding);
	std::vector<Pire::wchar32> ucs4;
	encoding.FromLocal(regexp, regexp + strlen(regexp), std::back_inserter(ucs4));
	lexer.Assign(ucs4.begin(), ucs4.end());
	Pire::Fsm fsm = lexer.Parse();
	fsm.Surround();
	return fsm.Compile<Pire::SlowCapturingScanner>();
}

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

static void TestRunner()
{
	const Pire::SlowCapturingScanner lazy = SlowCompile(".*?id=(\\d+?)\\d*&", 1);
	Pire::Hip::SlowCaptureBatchRunner run(lazy);
	// the accessors follow Run() / RunLines()
	CHECK(Has(Thrown([&] { run.Hits(); }), "Hits() follows Run() or RunLines()"));
	CHECK(Has(Thrown([&] { run.Captured(0); }), "the accessors per string follow Run()"));
	CHECK(Has(Thrown([&] { run.HitText(); }), "HitText() follows RunLines()"));
	CHECK(Has(Thrown([&] { run.LineCount(); }), "LineCount() follows RunLines()"));
	// no strings, no bytes: zeros, no device
	run.Run(nullptr, nullptr, 0).Select();
	CHECK(run.HitCount() == 0 && run.Hits().empty() && run.HitSpans().empty());
	run.Run(std::vector<Pire::ystring>());
	CHECK(run.HitCount() == 0);
	run.RunLines("", 0);
	CHECK(run.LineCount() == 0 && run.HitCount() == 0 && run.Hits().empty() && run.HitSpans().empty());
	CHECK(run.HitText().empty() && run.HitTextOffsets() == U64s(1, 0) && run.HitText('|').empty());
	CHECK(Has(Thrown([&] { run.Begin(0); }), "the accessors per string follow Run()"));
	// what the library refuses before it touches a device
	run.RunLines(nullptr, 5);
	std::string what = Thrown([&] { run.Hits(); });
	CHECK(Has(what, "pire_hip_slow_capture_lines_gather: ") && Has(what, "size > 0 with null raw"));
	what = Thrown([&] { run.HitText(); });
	CHECK(Has(what, "pire_hip_slow_capture_lines_gather: ") && Has(what, "size > 0 with null raw"));
	const uint64_t down[3] = {0, 5, 3};
	run.Run("id=1&x", down, 2);
	CHECK(Has(Thrown([&] { run.Captured(1); }), "non-decreasing"));
	CHECK(Has(Thrown([&] { run.Hits(); }), "non-decreasing"));
	const uint64_t far[2] = {0, uint64_t(1) << 32};
	run.Run("x", far, 1);
	what = Thrown([&] { run.Matched(0); });
	CHECK(Has(what, "pire_hip_slow_capture_run: ") && Has(what, "2^32 - 1 bytes"));
	// a plain SlowScanner's Save() form has no actions: refused at construction
	Pire::Fsm plain = Pire::Lexer("a.{3}b", "a.{3}b" + 6).Parse();
	plain.Surround();
	const Pire::SlowScanner slow = plain.Compile<Pire::SlowScanner>();
	pire_hip_slow_capture_table* t = nullptr;
	const std::string blob = Pire::Hip::SavedBlob(slow);
	CHECK(pire_hip_slow_capture_table_create(blob.data(), blob.size(), &t) == PIRE_HIP_EFORMAT && !t);
}

int main()
{
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
	printf("OK(slow capture shim: %d checks)\n", g_checks);
	return 0;
}
