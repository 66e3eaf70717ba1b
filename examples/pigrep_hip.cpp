// pigrep on the MI355X: the reference's sample grep (samples/pigrep/pigrep.cpp) with its one-line-at-a-time
//     if (Pire::Runner(sc).Begin().Run(line).End()) print(line)
// loop (pigrep.cpp:38-45) replaced by ONE batched call on the GPU, raw bytes in, matching lines out.  Same command
// line, same output.
//
//   pigrep_hip [-i] [-u] [-x] [-e pattern | pattern] [file [file2...]]
//
// Everything before the scan (lexer, features, Surround, Compile) is the reference library, unchanged; the scan goes
// through include/pire_hip/batch_runner.hpp.  Several files are ONE call: they go into one buffer, and the device says which
// file every hit belongs to (FileSet, Files()).  tests/test_examples.py builds the reference's own pigrep next to this one and
// compares their outputs.
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire_hip/batch_runner.hpp>

namespace {

// The stream as it is, in one buffer: cutting it into lines (getline semantics: the newline is not part of the line, a
// trailing fragment without newline is a line, an empty stream has no lines), scanning them and picking the lines that
// matched all happen on the GPU; what comes back is the text of the hits, a newline behind each: the output itself.
void GrepStream(std::istream& in, const Pire::Hip::Table<Pire::Scanner>& table, const std::string& prefix)
{
	const std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
	if (raw.empty())
		return;
	Pire::Hip::BatchRunner<Pire::Scanner> run(table);
	const std::string& hits = run.Begin().RunLines(raw.data(), raw.size()).End().HitText();
	if (prefix.empty()) {
		std::cout.write(hits.data(), std::streamsize(hits.size()));
	} else {
		const std::vector<uint64_t>& offsets = run.HitTextOffsets();
		for (size_t k = 0; k + 1 < offsets.size(); ++k) {
			std::cout << prefix;
			std::cout.write(hits.data() + offsets[k], std::streamsize(offsets[k + 1] - offsets[k]));
		}
	}
	std::cout.flush();
}

// Several inputs: all of them in one buffer (FileSet: a delimiter behind a file that lacks one, so no line runs from one file
// into the next), ONE split + scan + hit list with the file of every hit (Files()), one gather of the hits' text.
void GrepFiles(const Pire::Hip::FileSet& set, const Pire::Hip::Table<Pire::Scanner>& table)
{
	const std::string& raw = set.Raw();
	if (raw.empty())
		return;
	Pire::Hip::BatchRunner<Pire::Scanner> run(table);
	run.Begin().RunLines(raw.data(), raw.size()).End().Files(set.Bytes());
	const std::string& hits = run.HitText();
	const std::vector<uint64_t>& offsets = run.HitTextOffsets();
	const std::vector<uint64_t>& files = run.HitFiles();
	for (size_t k = 0; k + 1 < offsets.size() && k < files.size(); ++k) {
		std::cout << set.Name(size_t(files[k])) << ": ";
		std::cout.write(hits.data() + offsets[k], std::streamsize(offsets[k + 1] - offsets[k]));
	}
	std::cout.flush();
}

void Usage()
{
	std::cerr << "pigrep_hip: print the lines a Pire regexp matches, scanning on the GPU\n"
	             "  pigrep_hip [-i] [-u] [-x] (-e PATTERN | PATTERN) [FILE...]\n"
	             "    -i  ignore case            -u  pattern and text are UTF-8\n"
	             "    -x  allow re1&re2 and ~re  -e  next argument is the pattern, even if it starts with '-'\n"
	             "  no FILE (or '-'): standard input; several FILEs: lines are prefixed with the file name\n";
	exit(1);
}

}  // namespace

int main(int argc, char** argv)
{
	try {
		Pire::Lexer lexer;
		std::string pattern;
		bool havePattern = false;
		int arg = 1;
		for (; arg < argc; ++arg) {
			const std::string a = argv[arg];
			if (a == "-i") {
				lexer.AddFeature(Pire::Features::CaseInsensitive());
			} else if (a == "-u") {
				lexer.SetEncoding(Pire::Encodings::Utf8());
			} else if (a == "-x") {
				lexer.AddFeature(Pire::Features::AndNotSupport());
			} else if (a == "-e" && arg + 1 < argc && !havePattern) {
				pattern = argv[++arg];
				havePattern = true;
			} else if (a.size() > 1 && a[0] == '-') {
				Usage();
			} else if (!havePattern) {
				pattern = a;
				havePattern = true;
			} else {
				break;
			}
		}
		if (!havePattern)
			Usage();

		// pigrep.cpp:88-94: decode the pattern with the lexer's encoding, parse, Surround, compile
		Pire::TVector<Pire::wchar32> ucs4;
		lexer.Encoding().FromLocal(pattern.data(), pattern.data() + pattern.size(), std::back_inserter(ucs4));
		lexer.Assign(ucs4.begin(), ucs4.end());
		Pire::Scanner sc = lexer.Parse().Surround().Compile<Pire::Scanner>();
		Pire::Hip::Table<Pire::Scanner> table(sc);   // one device table for every file

		std::ios_base::sync_with_stdio(false);
		if (arg >= argc) {
			GrepStream(std::cin, table, "");
		} else {
			// pigrep.cpp:93-108: "-" is stdin; lines are prefixed with "name: " only when several files are given
			const bool many = argc - arg > 1;
			Pire::Hip::FileSet set;
			for (; arg < argc; ++arg) {
				const std::string name = argv[arg];
				if (name == "-") {
					if (!many) {
						GrepStream(std::cin, table, "");
						continue;
					}
					const std::string raw((std::istreambuf_iterator<char>(std::cin)), std::istreambuf_iterator<char>());
					set.Add("(stdin)", raw.data(), raw.size());
					continue;
				}
				std::ifstream f(name.c_str());
				if (!f) {
					GrepFiles(set, table);   // (the hits of the files in front of it come out first, as they always did)
					throw std::runtime_error("cannot open file " + name);
				}
				if (!many) {
					GrepStream(f, table, std::string());
					continue;
				}
				const std::string raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
				set.Add(name, raw.data(), raw.size());
			}
			if (many)
				GrepFiles(set, table);
		}
		return 0;
	} catch (const std::exception& e) {
		std::cerr << "pigrep_hip: " << e.what() << std::endl;
		return 1;
	}
}
