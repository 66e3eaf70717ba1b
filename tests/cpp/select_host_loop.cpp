// What pire_hip_run_select replaces, timed in C++ (tools/select_case.py drives this program): for one resident batch
//   (a) the scan alone                                      BatchRunner::RunDevice*().End(), results left on the device
//   (b) pire_hip_run_select with out_hits + out_hit_masks   ... and the hits fetched to the host (count, then 8 * (1 + W) bytes a hit)
//   (c) the loop of INTEGRATION.md section 2 through the shim: the scan, States() (5 bytes per string over PCIe), then one
//       sc.Final / sc.AcceptedRegexps lookup per string on the host
// Medians of warmed repetitions, host wall clock around call + synchronise.  (b) and (c) must give the same hits.
//   select_host_loop <scanner blob> strided <n> <len> <seed> <plants file | -> <reps>
//   select_host_loop <scanner blob> offsets <text file> <offsets file (u64)> <reps>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include <pire/pire.h>
#include <pire_hip/batch_runner.hpp>

typedef Pire::Hip::BatchRunner<Pire::Scanner> Runner;

static std::string ReadFile(const char* path)
{
	std::ifstream in(path, std::ios::binary);
	if (!in)
		throw Pire::Error(std::string("cannot read ") + path);
	return std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

static double Median(std::vector<double> v)
{
	std::sort(v.begin(), v.end());
	return v[v.size() / 2];
}

static double Now()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv)
{
	try {
		if (argc < 6) {
			fprintf(stderr, "usage: see the head of tests/cpp/select_host_loop.cpp\n");
			return 2;
		}
		const std::string blob = ReadFile(argv[1]);
		Pire::Scanner sc;
		{
			std::istringstream in(blob);
			sc.Load(&in);
		}
		const bool strided = !strcmp(argv[2], "strided");
		size_t n = 0, len = 0;
		int reps = 0;
		Pire::Hip::DeviceBuffer dText, dOffs;
		if (strided) {
			if (argc < 8)
				return 2;
			n = strtoull(argv[3], nullptr, 10);
			len = strtoull(argv[4], nullptr, 10);
			const uint64_t seed = strtoull(argv[5], nullptr, 10);
			std::string plants;
			if (strcmp(argv[6], "-"))
				plants = ReadFile(argv[6]);
			reps = atoi(argv[7]);
			dText.Reserve(n * len);
			Pire::Hip::Check(pire_hip_corpus_fill(dText.Get(), seed, 0, n, len, len, plants.empty() ? nullptr : plants.data(), nullptr));
		} else {
			const std::string text = ReadFile(argv[3]), offs = ReadFile(argv[4]);
			reps = atoi(argv[5]);
			n = offs.size() / 8 - 1;
			dText.Reserve(text.size() + 256);
			dOffs.Reserve(offs.size());
			Pire::Hip::Check(pire_hip_copy_to_device(dText.Get(), text.data(), text.size(), nullptr));
			Pire::Hip::Check(pire_hip_copy_to_device(dOffs.Get(), offs.data(), offs.size(), nullptr));
		}
		Pire::Hip::Check(pire_hip_stream_synchronize(nullptr));
		Pire::Hip::Table<Pire::Scanner> table(sc);
		Pire::Hip::Check(pire_hip_table_upload(table.Handle()));
		const size_t words = pire_hip_table_mask_words(table.Handle());
		const uint32_t flags = PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END | PIRE_HIP_RUN_ON_DEVICE;
		const uint64_t* offsets = static_cast<const uint64_t*>(dOffs.Get());

		Runner run(table);
		auto scan = [&]() -> Runner& {
			return strided ? run.Begin().RunDeviceStrided(dText.Get(), n, len, len).End()
			               : run.Begin().RunDevice(dText.Get(), offsets, n).End();
		};
		Pire::Hip::DeviceBuffer dHits, dMasks, dCount;
		uint64_t* hits = static_cast<uint64_t*>(dHits.Reserve(n * 8));
		uint64_t* masks = static_cast<uint64_t*>(dMasks.Reserve(n * words * 8));
		uint64_t* count = static_cast<uint64_t*>(dCount.Reserve(8));
		std::vector<uint64_t> gotHits, gotMasks, loopHits, loopMasks;
		std::vector<double> ta, tb, tbDev, tc;
		for (int r = -3; r < reps; ++r) {
			// (a)
			double t0 = Now();
			scan().DeviceStateIndices();
			Pire::Hip::Check(pire_hip_stream_synchronize(nullptr));
			const double a = Now() - t0;
			// (b)
			t0 = Now();
			if (strided)
				Pire::Hip::Check(pire_hip_run_select_strided(table.Handle(), dText.Get(), n, len, len, flags, nullptr, nullptr, nullptr,
				                                             nullptr, nullptr, nullptr, hits, masks, n, count, nullptr));
			else
				Pire::Hip::Check(pire_hip_run_select(table.Handle(), dText.Get(), offsets, n, flags, nullptr, nullptr, nullptr, nullptr,
				                                     nullptr, nullptr, hits, masks, n, count, nullptr));
			Pire::Hip::Check(pire_hip_stream_synchronize(nullptr));
			const double bDev = Now() - t0;
			uint64_t k = 0;
			Pire::Hip::Check(pire_hip_copy_to_host(&k, count, 8, nullptr));
			Pire::Hip::Check(pire_hip_stream_synchronize(nullptr));
			gotHits.resize(k);
			gotMasks.resize(k * words);
			if (k) {
				Pire::Hip::Check(pire_hip_copy_to_host(gotHits.data(), hits, k * 8, nullptr));
				Pire::Hip::Check(pire_hip_copy_to_host(gotMasks.data(), masks, k * words * 8, nullptr));
				Pire::Hip::Check(pire_hip_stream_synchronize(nullptr));
			}
			const double b = Now() - t0;
			// (c)
			t0 = Now();
			const std::vector<Pire::Scanner::State>& st = scan().States();
			loopHits.clear();
			loopMasks.clear();
			for (size_t i = 0; i < n; ++i)
				if (sc.Final(st[i])) {
					auto ids = sc.AcceptedRegexps(st[i]);
					const size_t at = loopMasks.size();
					loopMasks.resize(at + words, 0);
					for (const size_t* p = ids.first; p != ids.second; ++p)
						loopMasks[at + *p / 64] |= uint64_t(1) << (*p % 64);
					loopHits.push_back(i);
				}
			const double c = Now() - t0;
			if (r >= 0) {
				ta.push_back(a);
				tb.push_back(b);
				tbDev.push_back(bDev);
				tc.push_back(c);
			}
		}
		const bool same = gotHits == loopHits && gotMasks == loopMasks;
		printf("{\"n\": %zu, \"hits\": %zu, \"hit_rate\": %.6f, \"scan_ms\": %.4f, \"run_select_ms\": %.4f, "
		       "\"run_select_on_device_ms\": %.4f, \"host_loop_ms\": %.4f, \"same_answer\": %s, \"kernel\": \"%s\", \"reps\": %d}\n",
		       n, gotHits.size(), n ? double(gotHits.size()) / double(n) : 0.0, Median(ta), Median(tb), Median(tbDev), Median(tc),
		       same ? "true" : "false", pire_hip_last_kernel(), reps);
		return same ? 0 : 1;
	} catch (const std::exception& e) {
		fprintf(stderr, "exception: %s\n", e.what());
		return 2;
	}
}
