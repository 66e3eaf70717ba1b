// BatchRunner::Select / Hits / HitMasks / HitCount / DeviceHits of include/pire_hip/batch_runner.hpp against the host loop they
// replace, in the reference's own vocabulary: for every string, Runner(sc).Begin().Run(str).End().State(), then
// sc.Final(st) and sc.AcceptedRegexps(st) (multi.h:143, 149-158) -- the loop of INTEGRATION.md section 2.
// Built like shim_test.cpp (tests/cpp/Makefile, into oracle/_ref/bin with the libraries it links).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire_hip/batch_runner.hpp>

static int g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static Pire::Scanner Compile(const char* re, bool surround)
{
	Pire::Fsm fsm = Pire::Lexer(re, re + strlen(re)).Parse();
	if (surround)
		fsm.Surround();
	return fsm.Compile<Pire::Scanner>();
}

struct Expected {
	std::vector<uint64_t> hits, masks;   // masks: `words` per hit
};

// the host loop: one Final / AcceptedRegexps lookup per string
static Expected HostLoop(const Pire::Scanner& sc, const std::vector<Pire::ystring>& strings, const std::vector<size_t>& want,
                         size_t words)
{
	Expected e;
	for (size_t i = 0; i < strings.size(); ++i) {
		Pire::Scanner::State st = Pire::Runner(sc).Begin().Run(strings[i]).End().State();
		std::vector<uint64_t> mask(words, 0);
		auto acc = sc.AcceptedRegexps(st);
		for (const size_t* r = acc.first; r != acc.second; ++r)
			mask[*r / 64] |= uint64_t(1) << (*r % 64);
		bool selected = false;
		if (want.empty())
			selected = sc.Final(st);
		for (size_t k = 0; k < want.size(); ++k)
			if (want[k] < sc.RegexpsCount() && ((mask[want[k] / 64] >> (want[k] % 64)) & 1))
				selected = true;
		if (selected) {
			e.hits.push_back(i);
			e.masks.insert(e.masks.end(), mask.begin(), mask.end());
		}
	}
	return e;
}

static void Compare(const Pire::Scanner& sc, const std::vector<Pire::ystring>& strings)
{
	const size_t words = sc.RegexpsCount() > 64 ? (sc.RegexpsCount() + 63) / 64 : 1;
	std::vector<std::vector<size_t>> wants = {{}, {0}, {sc.RegexpsCount() - 1}, {0, 1, 2}, {sc.RegexpsCount() + 5}};
	Pire::Hip::Table<Pire::Scanner> table(sc);
	// host pointers
	Pire::Hip::BatchRunner<Pire::Scanner> gpu(table);
	gpu.Begin().Run(strings).End();
	CHECK(gpu.MaskWords() == words);
	for (const auto& want : wants) {
		const Expected e = HostLoop(sc, strings, want, words);
		gpu.Select(want);
		CHECK(gpu.HitCount() == e.hits.size());
		CHECK(gpu.Hits() == e.hits);
		CHECK(gpu.HitMasks() == e.masks);
	}
	// the same text resident on the device
	std::string flat;
	std::vector<uint64_t> offs(1, 0);
	for (const auto& s : strings) {
		flat.append(s.data(), s.size());
		offs.push_back(flat.size());
	}
	Pire::Hip::DeviceBuffer dText, dOffs;
	dText.Reserve(flat.size() + 256);
	dOffs.Reserve(offs.size() * 8);
	Pire::Hip::Check(pire_hip_copy_to_device(dText.Get(), flat.data(), flat.size(), nullptr));
	Pire::Hip::Check(pire_hip_copy_to_device(dOffs.Get(), offs.data(), offs.size() * 8, nullptr));
	Pire::Hip::Check(pire_hip_stream_synchronize(nullptr));
	Pire::Hip::BatchRunner<Pire::Scanner> dev(table);
	dev.Begin().RunDevice(dText.Get(), static_cast<const uint64_t*>(dOffs.Get()), strings.size()).End();
	for (const auto& want : wants) {
		const Expected e = HostLoop(sc, strings, want, words);
		dev.Select(want);
		CHECK(dev.Hits() == e.hits);
		CHECK(dev.HitMasks() == e.masks);
		CHECK(dev.HitCount() == e.hits.size());
		// where a consumer on the GPU finds them
		std::vector<uint64_t> raw(e.hits.size());
		uint64_t count = ~uint64_t(0);
		Pire::Hip::Check(pire_hip_copy_to_host(&count, dev.DeviceHitCount(), 8, nullptr));
		if (!raw.empty())
			Pire::Hip::Check(pire_hip_copy_to_host(raw.data(), dev.DeviceHits(), raw.size() * 8, nullptr));
		Pire::Hip::Check(pire_hip_stream_synchronize(nullptr));
		CHECK(count == e.hits.size() && raw == e.hits);
	}
}

int main()
{
	try {
		std::vector<Pire::ystring> text = {
			"def abc ghi", "abc", "def abd ghi", "abc ghi", "def abc", "xaez", "xadddddddddddez", "xx", "xxx", "", "hello world",
			"aaa", "bbb", "aaabbb", "ccc", "aaacccbbb", "HeadInnerInnerTail", Pire::ystring(3000, 'x') + "abc" + Pire::ystring(70, 'y'),
		};
		for (int i = 0; i < 700; ++i)   // more than one tile of the select pass, hits spread over its waves
			text.push_back(i % 7 == 0 ? "..aaa.." : i % 11 == 0 ? "bbbccc" : i % 13 == 0 ? "abc" : "nothing here");
		Pire::Scanner one = Compile("abc", true);
		Compare(one, text);
		Pire::Scanner glued = Pire::Scanner::Glue(Pire::Scanner::Glue(Compile("aaa", true), Compile("bbb", true)), Compile("ccc", true));
		CHECK(glued.RegexpsCount() == 3);
		Compare(glued, text);
		// more than 64 regexps: two mask words
		const char* letters = "abcdefghij";
		Pire::Scanner many;
		size_t count = 0;
		for (int a = 0; a < 10; ++a)
			for (int b = 0; b < 7; ++b) {
				const char re[3] = {letters[a], letters[b], 0};
				Pire::Scanner sc = Compile(re, false);
				many = count++ ? Pire::Scanner::Glue(many, sc) : sc;
			}
		CHECK(many.RegexpsCount() == 70 && !many.Empty());
		std::vector<Pire::ystring> pairs;
		for (int i = 0; i < 1500; ++i) {
			const char s[3] = {letters[(i * 7) % 10], letters[(i * 3) % 10], 0};
			pairs.push_back(i % 5 == 0 ? Pire::ystring("zz") : Pire::ystring(s));
		}
		Compare(many, pairs);
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	if (g_fail) {
		fprintf(stderr, "%d of %d checks FAILED\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(select shim: %d checks)\n", g_checks);
	return 0;
}
