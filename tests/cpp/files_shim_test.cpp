// Files() of BatchRunner, SlowBatchRunner and LineMatcher, and FileSet (include/pire_hip/batch_runner.hpp) as far as it is decided
// before a device is touched: what the library refuses comes back as Pire::Error with the entry point's name in it, a buffer
// of no bytes answers zeros and lists every file as one without a hit, Files() after anything but RunLines() throws, and
// FileSet appends the delimiter only where it is missing.  Fsms built as easy.h builds them, against the unmodified reference
// headers; into oracle/_ref/bin with the libraries it links.  It needs no GPU and is run without one.
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

// a runner with a buffer of no bytes behind RunLines() and a Files() of `files` empty files: zeros from every accessor, and
// every file is one without a hit
template <class Runner>
static void CheckEmpty(Runner& run, size_t files)
{
	CHECK(run.FileHitCounts() == U64s(files, 0));
	CHECK(run.FilesWithHits().empty());
	CHECK(run.HitFiles().empty() && run.HitFileLines().empty());
	CHECK(run.FileLines() == U64s(files + 1, 0));
	CHECK(run.Straddles() == 0);
	U64s all(files);
	for (size_t f = 0; f < files; ++f)
		all[f] = f;
	CHECK(run.FilesWithoutHits() == all);
}

static void TestFileSet()
{
	Pire::Hip::FileSet set;
	CHECK(set.Raw().empty() && set.Bytes() == U64s(1, 0) && set.Size() == 0);
	set.Add("empty", "", 0);
	set.Add("ends in newline", "ab\ncd\n", 6);
	set.Add("does not", "ef\ngh", 5);
	set.Add("one empty line", "\n", 1);
	set.Add("empty again", nullptr, 0);
	set.Add("one byte", "x", 1);
	CHECK(set.Raw() == "ab\ncd\nef\ngh\n\nx\n");
	const uint64_t bytes[] = {0, 0, 6, 12, 13, 13, 15};
	CHECK(set.Bytes() == U64s(bytes, bytes + 7));
	CHECK(set.Size() == 6 && set.Name(0) == "empty" && set.Name(2) == "does not" && set.Name(5) == "one byte");
	// every boundary inside the buffer follows a delimiter: nothing straddles
	for (size_t f = 1; f < set.Size(); ++f)
		CHECK(set.Bytes()[f] == 0 || set.Raw()[set.Bytes()[f] - 1] == '\n');
	Pire::Hip::FileSet bars('|');
	bars.Add("a", "x|y", 3);
	bars.Add("b", "z|", 2);
	CHECK(bars.Raw() == "x|y|z|" && bars.Bytes()[1] == 4 && bars.Bytes()[2] == 6);
}

static void TestFastRunner()
{
	const Pire::Scanner sc = Surrounded("a.{3}b").Compile<Pire::Scanner>();
	Pire::Hip::BatchRunner<Pire::Scanner> gpu(sc);
	const std::vector<Pire::ystring> none;
	const U64s noFiles(1, 0), three(4, 0);
	// Files() follows RunLines(), and nothing else
	CHECK(Has(Thrown([&] { gpu.Files(three); }), "Files() follows RunLines()"));
	gpu.Begin().Run(none).End();
	CHECK(Has(Thrown([&] { gpu.Files(three); }), "Files() follows RunLines()"));
	gpu.Begin().RunLinesField("", 0, 1).End();
	CHECK(Has(Thrown([&] { gpu.Files(three); }), "Files() follows RunLines()"));
	// the accessors follow Files()
	gpu.Begin().RunLines("", 0).End();
	CHECK(Has(Thrown([&] { gpu.FileHitCounts(); }), "FileHitCounts() follows Files()"));
	CHECK(Has(Thrown([&] { gpu.FilesWithoutHits(); }), "FilesWithoutHits() follows Files()"));
	CHECK(Has(Thrown([&] { gpu.Straddles(); }), "Straddles() follows Files()"));
	// no bytes: every file is empty
	gpu.Files(three);
	CheckEmpty(gpu, 3);
	gpu.Files(noFiles);
	CheckEmpty(gpu, 0);
	gpu.Files(U64s());   // (no boundaries at all: no files)
	CheckEmpty(gpu, 0);
	// a selection keeps the request, a batch ends it
	gpu.Files(three).Select();
	CheckEmpty(gpu, 3);
	gpu.Begin().RunLines("", 0).End();
	CHECK(Has(Thrown([&] { gpu.HitFiles(); }), "HitFiles() follows Files()"));
	// what the library refuses before it touches a device
	gpu.Begin().RunLines(nullptr, 5).End().Files(three);
	std::string what = Thrown([&] { gpu.FileHitCounts(); });
	CHECK(Has(what, "pire_hip_run_lines_files_select") && Has(what, "size > 0 with null raw"));
	const uint64_t down[] = {0, 4, 2, 5}, late[] = {1, 2, 4, 5}, shortOf[] = {0, 2, 4, 4};
	gpu.Begin().RunLines("ab\ncd", 5).End().Files(U64s(down, down + 4));
	what = Thrown([&] { gpu.FilesWithHits(); });
	CHECK(Has(what, "pire_hip_run_lines_files_select") && Has(what, "file_bytes must be non-decreasing"));
	gpu.Files(U64s(late, late + 4));
	CHECK(Has(Thrown([&] { gpu.FilesWithoutHits(); }), "file_bytes[0] != 0"));
	gpu.Files(U64s(shortOf, shortOf + 4));
	CHECK(Has(Thrown([&] { gpu.HitFileLines(); }), "file_bytes[files] != size"));
	gpu.Files(noFiles);
	CHECK(Has(Thrown([&] { gpu.FileLines(); }), "files == 0 with size > 0"));
	// the hit accessors of RunLines() are what they were
	gpu.Begin().RunLines("", 0).End().Files(three);
	CHECK(gpu.LineCount() == 0 && gpu.HitCount() == 0 && gpu.HitText().empty());
	CheckEmpty(gpu, 3);
}

static void TestSlowRunner()
{
	const Pire::SlowScanner sc = Surrounded("a.{20}$").Compile<Pire::SlowScanner>();
	Pire::Hip::SlowBatchRunner gpu(sc);
	const std::vector<Pire::ystring> none;
	const U64s two(3, 0);
	CHECK(Has(Thrown([&] { gpu.Files(two); }), "Files() follows RunLines()"));
	gpu.Run(none);
	CHECK(Has(Thrown([&] { gpu.Files(two); }), "Files() follows RunLines()"));
	for (int invert = 0; invert < 2; ++invert) {
		gpu.RunLines("", 0, '\n', invert != 0);
		CHECK(Has(Thrown([&] { gpu.FilesWithHits(); }), "FilesWithHits() follows Files()"));
		gpu.Files(two);
		CheckEmpty(gpu, 2);
		gpu.Select(invert == 0);   // (honoured: the request stays, the lists are fetched anew)
		CheckEmpty(gpu, 2);
	}
	gpu.RunLines(nullptr, 5).Files(two);
	std::string what = Thrown([&] { gpu.FileHitCounts(); });
	CHECK(Has(what, "pire_hip_slow_lines_files_select") && Has(what, "size > 0 with null raw"));
	const uint64_t down[] = {0, 3, 2};
	gpu.RunLines("ab", 2).Files(U64s(down, down + 3));
	what = Thrown([&] { gpu.FilesWithoutHits(); });
	CHECK(Has(what, "pire_hip_slow_lines_files_select") && Has(what, "file_bytes"));
}

static void TestLineMatcher()
{
	Pire::Hip::LineMatcher fast(Surrounded("a.{3}b"));
	Pire::Hip::LineMatcher slow(Surrounded("a.{20}$"));   // 2^21 subsets: Fsm::Determine() gives up
	CHECK(!fast.IsSlow() && slow.IsSlow());
	Pire::Hip::LineMatcher* both[2] = {&fast, &slow};
	const U64s five(6, 0);
	for (int k = 0; k < 2; ++k) {
		Pire::Hip::LineMatcher& m = *both[k];
		CHECK(Has(Thrown([&] { m.Files(five); }), "Files() follows RunLines()"));
		m.RunLines("", 0).Files(five);
		CheckEmpty(m, 5);
		m.RunLines(nullptr, 5).Files(five);
		CHECK(Has(Thrown([&] { m.FileHitCounts(); }), "size > 0 with null raw"));
		CHECK(Has(Thrown([&] { m.FilesWithoutHits(); }), "size > 0 with null raw"));
	}
	slow.RunLines("", 0, '\n', true).Files(five);
	CheckEmpty(slow, 5);
}

int main()
{
	// the C ABI itself, as a caller in C++ sees it: codes and names
	uint64_t count = 77, lines = 77, hitCount = 77, straddles = 77;
	uint64_t first[4] = {9, 9, 9, 9}, listed[4] = {9, 9, 9, 9}, hitFile[3] = {9, 9, 9}, hitLine[3] = {9, 9, 9};
	const uint64_t hits[3] = {1, 4, 6}, unsorted[3] = {4, 1, 6}, bounds[4] = {0, 2, 2, 8}, down[4] = {0, 5, 2, 8}, late[4] = {1, 2, 2, 8};
	CHECK(pire_hip_files(hits, nullptr, 3, 8, bounds, 3, 0, 0, first, hitFile, hitLine, listed, 4, nullptr, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_files: null out_file_count") == 0);
	CHECK(pire_hip_files(nullptr, nullptr, 3, 8, bounds, 3, 0, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_files: hit_cap > 0 with null hits") == 0);
	CHECK(pire_hip_files(hits, nullptr, 3, 8, nullptr, 3, 0, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_files: files > 0 with null bounds") == 0);
	CHECK(pire_hip_files(hits, nullptr, 3, 8, bounds, 3, 0, 0, first, hitFile, hitLine, nullptr, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_files: file_cap > 0 with null out_files") == 0);
	CHECK(pire_hip_files(hits, nullptr, 3, 8, bounds, 3, 2, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_files: unknown file_mode") == 0);
	CHECK(pire_hip_files(hits, nullptr, 3, 8, nullptr, 0, 0, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_files: files == 0 with n > 0") == 0);
	CHECK(pire_hip_files(hits, nullptr, 3, uint64_t(1) << 32, bounds, 3, 0, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_files(hits, nullptr, uint64_t(1) << 32, 8, bounds, 3, 0, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(pire_hip_files(hits, nullptr, 3, 8, bounds, uint64_t(1) << 32, 0, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	// host pointers: the list and the bounds are looked at before anything is written
	CHECK(pire_hip_files(unsorted, nullptr, 3, 8, bounds, 3, 0, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_files: hits must be strictly ascending") == 0);
	CHECK(pire_hip_files(hits, nullptr, 3, 6, bounds, 3, 0, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_files: hit out of range") == 0);
	CHECK(pire_hip_files(hits, nullptr, 3, 8, down, 3, 0, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_files: bounds must be non-decreasing") == 0);
	CHECK(pire_hip_files(hits, nullptr, 3, 8, late, 3, 0, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_files: bounds[0] != 0") == 0);
	CHECK(pire_hip_files(hits, nullptr, 3, 9, bounds, 3, 0, 0, first, hitFile, hitLine, listed, 4, &count, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_files: bounds[files] != n") == 0);
	CHECK(count == 77 && first[0] == 9 && listed[0] == 9 && hitFile[0] == 9 && hitLine[0] == 9);
	// no files: zeros, no device is touched
	CHECK(pire_hip_files(nullptr, nullptr, 0, 0, nullptr, 0, PIRE_HIP_FILES_WITHOUT, 0, first, nullptr, nullptr, nullptr, 0, &count, nullptr) == PIRE_HIP_OK);
	CHECK(count == 0 && first[0] == 0 && first[1] == 9);
	// the lines forms
	count = 77;
	CHECK(pire_hip_run_lines_files_select(nullptr, "a\n", 2, '\n', 0, nullptr, bounds, 3, 0, &lines, nullptr, nullptr, nullptr, nullptr, 0, &hitCount,
	                                      nullptr, nullptr, nullptr, 0, &count, &straddles, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_run_lines_files_select: null table") == 0);
	CHECK(pire_hip_slow_lines_files_select(nullptr, "a\n", 2, '\n', 0, 0, bounds, 3, 0, &lines, nullptr, nullptr, nullptr, nullptr, 0, &hitCount,
	                                       nullptr, nullptr, nullptr, 0, &count, &straddles, nullptr) == PIRE_HIP_EINVAL);
	CHECK(std::string(pire_hip_last_error()).find("pire_hip_slow_lines_files_select: null table") == 0);
	CHECK(lines == 77 && hitCount == 77 && count == 77 && straddles == 77);
	try {
		TestFileSet();
		TestFastRunner();
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
	printf("OK(files shim: %d checks)\n", g_checks);
	return 0;
}
