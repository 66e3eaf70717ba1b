// CaptureBatchRunner::RunLines(...).CapturedText() (include/pire_hip/batch_runner.hpp) against the UNMODIFIED reference:
// the strings of tests/capture_ut.cpp:93-129 and mixtures of them, joined by newlines, must give exactly the captured
// fields that Pire::CapturingScanner yields line by line through the reference's own helper (capture_ut.cpp:85-91).
// Compiled by tests/test_capture_select.py where the reference tree exists, into oracle/_ref/bin.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire/extra.h>
#include <pire_hip/batch_runner.hpp>

static int g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

int main()
{
	try {
		const char* regexp = "google_id\\s*=\\s*[\'\"]([a-z0-9]+)[\'\"]\\s*;";
		Pire::Lexer lexer;
		lexer.Assign(regexp, regexp + strlen(regexp));
		lexer.AddFeature(Pire::Features::Capture(1));
		Pire::Fsm fsm = lexer.Parse();
		fsm.Surround();
		fsm.Determine();
		Pire::CapturingScanner sc = fsm.Compile<Pire::CapturingScanner>();
		const char* fixed[] = {"google_id = 'abcde';", "var google_id = 'abcde'; eval(google_id);", "google_id != 'abcde';",
		                       "google_id = 'abcde'; google_id = 'xyz';", "var google_id = 'abc de'; google_id = 'xyz';", ""};
		std::vector<std::string> lines(fixed, fixed + sizeof(fixed) / sizeof(fixed[0]));
		unsigned seed = 7;
		for (int i = 0; i < 3000; ++i) {
			std::string s;
			for (int part = 0; part < 3; ++part) {
				seed = seed * 1103515245u + 12345u;
				if ((seed >> 16) & 1)
					s += fixed[(seed >> 17) % 5];
				else
					s += std::string((seed >> 17) % 23, char('a' + (seed >> 22) % 26));
			}
			lines.push_back(s);
		}
		std::string raw;
		for (size_t i = 0; i < lines.size(); ++i)
			raw += lines[i] + (i + 1 < lines.size() ? "\n" : "");   // no newline behind the last line
		// the reference, line by line
		std::string want;
		std::vector<uint64_t> wantLines, wantSpans;
		uint64_t at = 0;
		for (size_t i = 0; i < lines.size(); ++i) {
			Pire::CapturingScanner::State st;
			sc.Initialize(st);
			Pire::Step(sc, st, Pire::BeginMark);
			Pire::Run(sc, st, lines[i].data(), lines[i].data() + lines[i].size());
			Pire::Step(sc, st, Pire::EndMark);
			if (st.Captured()) {
				want += std::string(lines[i].data() + st.Begin() - 1, lines[i].data() + st.End() - 1) + "\n";
				wantLines.push_back(i);
				wantSpans.push_back(at + st.Begin() - 1);
				wantSpans.push_back(at + st.End() - 1);
			}
			at += lines[i].size() + 1;
		}
		CHECK(wantLines.size() > 100 && wantLines.size() < lines.size());
		Pire::Hip::CaptureBatchRunner gpu(sc);
		gpu.Begin().RunLines(raw.data(), raw.size()).End();
		CHECK(gpu.CapturedText() == want);
		CHECK(gpu.CapturedLines() == wantLines);
		CHECK(gpu.CapturedSpans() == wantSpans);
		CHECK(gpu.LineCount() == lines.size());
		const std::vector<uint64_t>& o = gpu.CapturedTextOffsets();
		CHECK(o.size() == wantLines.size() + 1 && o.back() == want.size());
		for (size_t k = 0; k + 1 < o.size(); ++k)
			CHECK(want.compare(o[k], o[k + 1] - o[k] - 1, raw, wantSpans[2 * k], wantSpans[2 * k + 1] - wantSpans[2 * k]) == 0);
		// the list alone, asked for first; then an offset batch of the same strings
		Pire::Hip::CaptureBatchRunner again(sc);
		again.Begin().RunLines(raw.data(), raw.size()).End();
		CHECK(again.CapturedSpans() == wantSpans && again.CapturedLines() == wantLines);
		CHECK(again.CapturedText('\0').size() == want.size());
		std::vector<Pire::ystring> strings(lines.begin(), lines.end());
		again.Run(strings);
		std::vector<uint64_t> batchSpans;
		at = 0;
		for (size_t i = 0, k = 0; i < lines.size(); ++i) {
			if (k < wantLines.size() && wantLines[k] == i) {
				batchSpans.push_back(wantSpans[2 * k] - i);      // no delimiters in a batch
				batchSpans.push_back(wantSpans[2 * k + 1] - i);
				++k;
			}
		}
		CHECK(again.CapturedSpans() == batchSpans && again.CapturedLines() == wantLines);
		CHECK(again.Captured(0) && !again.Captured(2));
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	if (g_fail) {
		fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(capture lines: %d checks)\n", g_checks);
	return 0;
}
