// BatchRunner::Route / RouteCount / RouteHits / RouteSpans / DeviceRouteHits of include/pire_hip/batch_runner.hpp against the C
// calls they wrap (pire_hip_run_route, pire_hip_run_lines_route) and against the host loop they replace, in the reference's
// own vocabulary: for every string, Runner(sc).Begin().Run(str).End().State(), then sc.AcceptedRegexps(st)
// (multi.h:149-158), bucketed by regexp.  Built like shim_test.cpp, into oracle/_ref/bin with the libraries it links.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire_hip/batch_runner.hpp>

static int g_checks = 0, g_fail = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

typedef std::vector<std::vector<uint64_t> > Rows;

static Pire::Scanner Compile(const char* re)
{
	Pire::Fsm fsm = Pire::Lexer(re, re + strlen(re)).Parse();
	fsm.Surround();
	return fsm.Compile<Pire::Scanner>();
}

// the host loop: one AcceptedRegexps lookup per string, bucketed by regexp
static Rows HostLoop(const Pire::Scanner& sc, const std::vector<Pire::ystring>& strings)
{
	Rows rows(sc.RegexpsCount());
	for (size_t i = 0; i < strings.size(); ++i) {
		Pire::Scanner::State st = Pire::Runner(sc).Begin().Run(strings[i]).End().State();
		auto acc = sc.AcceptedRegexps(st);
		for (const size_t* r = acc.first; r != acc.second; ++r)
			rows[*r].push_back(i);
	}
	return rows;
}

static void Compare(const Pire::Scanner& sc, const std::vector<Pire::ystring>& strings)
{
	const size_t regexps = sc.RegexpsCount(), n = strings.size();
	const Rows want = HostLoop(sc, strings);
	Pire::Hip::Table<Pire::Scanner> table(sc);
	std::string flat, raw;
	std::vector<uint64_t> offs(1, 0), begins;
	for (size_t i = 0; i < n; ++i) {
		flat.append(strings[i].data(), strings[i].size());
		offs.push_back(flat.size());
		begins.push_back(raw.size());
		raw.append(strings[i].data(), strings[i].size());
		raw.push_back('\n');
	}
	const uint32_t be = PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END;

	// the C call on host pointers
	std::vector<uint64_t> counts(regexps, ~uint64_t(0)), hits(regexps * n);
	Pire::Hip::Check(pire_hip_run_route(table.Handle(), flat.data(), offs.data(), n, be, nullptr, nullptr, nullptr, nullptr, hits.data(), n,
	                                    counts.data(), nullptr));
	// Route() after Run().End(): host pointers
	Pire::Hip::BatchRunner<Pire::Scanner> gpu(table);
	gpu.Begin().Run(strings).End().Route();
	for (size_t r = 0; r < regexps; ++r) {
		CHECK(gpu.RouteCount(r) == want[r].size() && counts[r] == want[r].size());
		CHECK(gpu.RouteHits(r) == want[r]);
		CHECK(std::vector<uint64_t>(hits.begin() + r * n, hits.begin() + r * n + counts[r]) == want[r]);
	}
	CHECK(gpu.States().size() == n);   // the per-string accessors keep working beside it

	// ... the same text resident on the device, the rows left where a consumer on the GPU wants them
	Pire::Hip::DeviceBuffer dText, dOffs;
	dText.Reserve(flat.size() + 256);
	dOffs.Reserve(offs.size() * 8);
	Pire::Hip::Check(pire_hip_copy_to_device(dText.Get(), flat.data(), flat.size(), nullptr));
	Pire::Hip::Check(pire_hip_copy_to_device(dOffs.Get(), offs.data(), offs.size() * 8, nullptr));
	Pire::Hip::Check(pire_hip_stream_synchronize(nullptr));
	Pire::Hip::BatchRunner<Pire::Scanner> dev(table);
	dev.Begin().RunDevice(dText.Get(), static_cast<const uint64_t*>(dOffs.Get()), n).End().Route();
	CHECK(dev.RoutePitch() == n);
	std::vector<uint64_t> devCounts(regexps), devHits(regexps * n);
	Pire::Hip::Check(pire_hip_copy_to_host(devCounts.data(), dev.DeviceRouteCounts(), regexps * 8, nullptr));
	Pire::Hip::Check(pire_hip_copy_to_host(devHits.data(), dev.DeviceRouteHits(), regexps * n * 8, nullptr));
	Pire::Hip::Check(pire_hip_stream_synchronize(nullptr));
	for (size_t r = 0; r < regexps; ++r) {
		CHECK(devCounts[r] == want[r].size());
		CHECK(std::vector<uint64_t>(devHits.begin() + r * n, devHits.begin() + r * n + want[r].size()) == want[r]);
		CHECK(dev.RouteHits(r) == want[r] && dev.RouteCount(r) == want[r].size());
	}

	// Route() after RunLines(): against the C call, and the spans against the lines themselves
	uint64_t lineCount = 0;
	std::vector<uint64_t> lcounts(regexps), lhits(regexps * n), lspans(regexps * n * 2);
	Pire::Hip::Check(pire_hip_run_lines_route(table.Handle(), raw.data(), raw.size(), '\n', be, &lineCount, lhits.data(), lspans.data(), n,
	                                          lcounts.data(), nullptr));
	CHECK(lineCount == n);
	Pire::Hip::BatchRunner<Pire::Scanner> lines(table);
	lines.Begin().RunLines(raw.data(), raw.size()).End().Route();
	CHECK(lines.LineCount() == n);
	for (size_t r = 0; r < regexps; ++r) {
		CHECK(lcounts[r] == want[r].size() && lines.RouteCount(r) == want[r].size());
		CHECK(lines.RouteHits(r) == want[r]);
		CHECK(std::vector<uint64_t>(lhits.begin() + r * n, lhits.begin() + r * n + lcounts[r]) == want[r]);
		const std::vector<uint64_t>& spans = lines.RouteSpans(r);
		CHECK(spans.size() == 2 * want[r].size());
		CHECK(std::vector<uint64_t>(lspans.begin() + 2 * r * n, lspans.begin() + 2 * (r * n + lcounts[r])) == spans);
		bool same = spans.size() == 2 * want[r].size();
		for (size_t k = 0; same && k < want[r].size(); ++k) {
			const size_t i = want[r][k];
			same = spans[2 * k] == begins[i] && spans[2 * k + 1] == begins[i] + strings[i].size();
		}
		CHECK(same);
	}
}

int main()
{
	try {
		std::vector<Pire::ystring> text = {
			"def abc ghi", "abc", "aaa", "bbb", "aaabbb", "ccc", "aaacccbbb", "", "xx", Pire::ystring(3000, 'x') + "abc" + Pire::ystring(70, 'y'),
		};
		for (int i = 0; i < 2300; ++i)   // more than two tiles of the route pass, every row spread over their waves
			text.push_back(i % 7 == 0 ? "..aaa.." : i % 11 == 0 ? "bbbccc" : i % 13 == 0 ? "abc aaa bbb ccc" : "nothing here");
		Compare(Compile("abc"), text);
		Pire::Scanner glued = Pire::Scanner::Glue(Pire::Scanner::Glue(Compile("aaa"), Compile("bbb")), Compile("ccc"));
		glued = Pire::Scanner::Glue(glued, Compile("abc"));
		CHECK(glued.RegexpsCount() == 4);
		Compare(glued, text);
		// few lines, many of them hits: RunLines().Route() has to grow its rows and call again
		std::vector<Pire::ystring> dense(3000, Pire::ystring("aaa"));
		Compare(glued, dense);
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
	if (g_fail) {
		fprintf(stderr, "%d of %d checks FAILED\n", g_fail, g_checks);
		return 1;
	}
	printf("OK(route shim: %d checks)\n", g_checks);
	return 0;
}
