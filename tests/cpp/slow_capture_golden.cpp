// What Pire::SlowCapturingScanner answers, as data: the generator of tests/golden/slow_capture (driver:
// tests/golden/make_slow_capture_inputs.py) and the yardstick of tools/slow_capture_case.py.  Compiled against the unmodified
// reference headers into oracle/_ref/bin; a scanner is built as the reference's own capture test builds one (Features::Capture,
// UTF-8, Surround(), Compile<SlowCapturingScanner>) and run as it runs one (Initialize + Run, no marks stepped by hand).
//
//   slow_capture_golden gen REQUEST OUTDIR
//       REQUEST: lines `case NAME INDEX PATTERN-HEX`, then one `s [HEX]` per string, then `end`; any number of cases.
//       Writes OUTDIR/NAME.blob (Save()) and prints per case `case NAME states letters start`, per string
//       `r captured begin end matched live` (begin / end: -1 for npos and where GetCapture assigned nothing; live: the longest
//       state list the walk held, Initialize's included), and `end`.
//   slow_capture_golden --time PATTERN-HEX INDEX FILE [REPEAT]
//       Runs the scanner over every '\n'-terminated line of FILE on one core, REPEAT times (default 1), and prints
//       `lines bytes captured seconds sum` of the last repeat (sum: of begin + end over the lines that captured).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire/extra.h>

typedef Pire::SlowCapturingScanner Slow;

static std::string FromHex(const std::string& hex)
{
	std::string out;
	for (size_t i = 0; i + 1 < hex.size(); i += 2)
		out.push_back(char(strtoul(hex.substr(i, 2).c_str(), nullptr, 16)));
	return out;
}

static Slow SlowCompile(const std::string& regexp, size_t index)
{
	const Pire::Encoding& encoding = Pire::Encodings::Utf8();
	Pire::Lexer lexer;
	lexer.AddFeature(Pire::Features::Capture(index));
	lexer.SetEncoding(encoding);
	std::vector<Pire::wchar32> ucs4;
	encoding.FromLocal(regexp.data(), regexp.data() + regexp.size(), std::back_inserter(ucs4));
	lexer.Assign(ucs4.begin(), ucs4.end());
	Pire::Fsm fsm = lexer.Parse();
	fsm.Surround();
	return fsm.Compile<Slow>();
}

struct Answer {
	int captured, matched;
	long long begin, end;
};

static Answer Ask(const Slow& sc, const char* b, const char* e)
{
	Slow::State st;
	sc.Initialize(st);
	Pire::Run(sc, st, b, e);
	Slow::SingleState fin;
	// (a SingleState of its own says npos / npos: whether GetCapture assigned is read off a state it cannot leave)
	Slow::SingleState untouched(size_t(-2));
	fin = untouched;
	Answer a;
	a.captured = sc.GetCapture(st, fin) ? 1 : 0;
	a.matched = fin.GetNum() != size_t(-2) ? 1 : 0;
	a.begin = a.matched && fin.HasBegin() ? (long long)fin.GetBegin() : -1;
	a.end = a.matched && fin.HasEnd() ? (long long)fin.GetEnd() : -1;
	return a;
}

static size_t Live(const Slow& sc, const std::string& s)
{
	Slow::State st;
	sc.Initialize(st);
	size_t live = st.GetSize();
	for (size_t i = 0; i < s.size(); ++i) {
		sc.Next(st, Pire::Char((unsigned char)s[i]));
		if (st.GetSize() > live)
			live = st.GetSize();
	}
	return live;
}

static int Generate(const char* request, const std::string& outdir)
{
	std::ifstream in(request);
	if (!in) {
		fprintf(stderr, "cannot read %s\n", request);
		return 2;
	}
	std::string line;
	std::unique_ptr<Slow> held;   // (the scanner has a const member: it cannot be assigned)
	bool open = false;
	while (std::getline(in, line)) {
		std::istringstream f(line);
		std::string word;
		f >> word;
		if (word == "case") {
			std::string name, hex;
			size_t index = 0;
			f >> name >> index >> hex;
			held.reset(new Slow(SlowCompile(FromHex(hex), index)));
			const Slow& sc = *held;
			std::ostringstream blob;
			sc.Save(&blob);
			std::ofstream out((outdir + "/" + name + ".blob").c_str(), std::ios::binary);
			const std::string bytes = blob.str();
			out.write(bytes.data(), std::streamsize(bytes.size()));
			unsigned long long start = 0;   // (GetStart() is protected: m.start as Save() wrote it, scanner_io.cpp:75)
			if (bytes.size() >= 48)
				memcpy(&start, bytes.data() + 40, 8);
			printf("case %s %zu %zu %llu\n", name.c_str(), sc.Size(), sc.GetLettersCount(), start);
			open = true;
		} else if (word == "s" && open) {
			std::string hex;
			f >> hex;
			const std::string s = FromHex(hex);
			const Slow& sc = *held;
			const Answer a = Ask(sc, s.data(), s.data() + s.size());
			printf("r %d %lld %lld %d %zu\n", a.captured, a.begin, a.end, a.matched, Live(sc, s));
		} else if (word == "end") {
			printf("end\n");
			open = false;
		}
	}
	return 0;
}

static int Time(const std::string& pattern, size_t index, const char* file, int repeat)
{
	std::ifstream in(file, std::ios::binary);
	if (!in) {
		fprintf(stderr, "cannot read %s\n", file);
		return 2;
	}
	const std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
	const Slow sc = SlowCompile(pattern, index);
	size_t lines = 0, captured = 0;
	unsigned long long sum = 0;
	double seconds = 0;
	for (int r = 0; r < repeat; ++r) {
		lines = captured = 0;
		sum = 0;
		const auto t0 = std::chrono::steady_clock::now();
		for (size_t b = 0; b < raw.size();) {
			size_t e = raw.find('\n', b);
			if (e == std::string::npos)
				e = raw.size();
			const Answer a = Ask(sc, raw.data() + b, raw.data() + e);
			++lines;
			if (a.captured) {
				++captured;
				sum += (unsigned long long)(a.begin + a.end);
			}
			b = e + 1;
		}
		seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	}
	printf("%zu %zu %zu %.6f %llu\n", lines, raw.size(), captured, seconds, sum);
	return 0;
}

int main(int argc, char** argv)
try {
	if (argc == 4 && !strcmp(argv[1], "gen"))
		return Generate(argv[2], argv[3]);
	if ((argc == 5 || argc == 6) && !strcmp(argv[1], "--time"))
		return Time(FromHex(argv[2]), size_t(atoi(argv[3])), argv[4], argc == 6 ? atoi(argv[5]) : 1);
	fprintf(stderr, "usage: %s gen REQUEST OUTDIR | --time PATTERN-HEX INDEX FILE [REPEAT]\n", argv[0]);
	return 2;
} catch (const std::exception& e) {
	fprintf(stderr, "exception: %s\n", e.what());
	return 3;
}
