// The blob parser and the host DFS of slow_capture.hip under AddressSanitizer + UndefinedBehaviorSanitizer, in a program of
// its own: create, get_info and image on every file given, and create on every prefix of it.  Host code only, run on the CPU.
//   make -C pire_amd/csrc asan                      # pire_amd/libpire_hip_asan.so: the library's host side, sanitized
//   CLANG=/opt/rocm/lib/llvm/bin/clang++            # the compiler hipcc drives: the same sanitizer runtime as the library's
//   $CLANG -fsanitize=address,undefined -shared-libsan -Iinclude tools/slow_capture_sanitize.cpp -Lpire_amd -lpire_hip_asan \
//          -Wl,-rpath,$PWD/pire_amd -Wl,-rpath,$(dirname $($CLANG -print-file-name=libclang_rt.asan-x86_64.so)) -o build/sanitize
//   build/sanitize tests/golden/slow_capture/*.blob
// The program itself is sanitized, so nothing is preloaded.  Exits 1 when a call answers what it must not.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "pire_hip.h"

int main(int argc, char** argv)
{
	int bad = 0;
	for (int a = 1; a < argc; ++a) {
		std::ifstream in(argv[a], std::ios::binary);
		const std::vector<char> blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
		pire_hip_slow_capture_table* t = nullptr;
		const int rc = pire_hip_slow_capture_table_create(blob.data(), blob.size(), &t);
		pire_hip_slow_capture_info info = {};
		if (rc == PIRE_HIP_OK) {
			bad += pire_hip_slow_capture_table_get_info(t, &info) != PIRE_HIP_OK;
			// exactly as large as the table says: a write past any of them is the sanitizer's to see
			std::vector<uint32_t> pos(size_t(info.states) * info.letters + 1), ent(info.entries);
			std::vector<uint8_t> flags(info.states), letters(260);
			std::vector<int64_t> init(size_t(info.init_len) * 3), match(3);
			bad += pire_hip_slow_capture_table_image(t, pos.data(), ent.data(), ent.size(), flags.data(), init.data(), match.data(),
			                                         letters.data()) != PIRE_HIP_OK;
			bad += pos.back() != info.entries;
			pire_hip_slow_capture_table_destroy(t);
		}
		size_t refused = 0;   // every prefix, each in a buffer of exactly its size: none of a good blob is one
		for (size_t cut = 0; cut < blob.size(); cut += (cut < 4096 || blob.size() - cut < 4096) ? 1 : 61) {
			const std::vector<char> part(blob.begin(), blob.begin() + cut);
			pire_hip_slow_capture_table* p = nullptr;
			if (pire_hip_slow_capture_table_create(part.data(), part.size(), &p) == PIRE_HIP_OK) {
				bad += rc == PIRE_HIP_OK;
				pire_hip_slow_capture_table_destroy(p);
			} else {
				++refused;
			}
		}
		printf("%-48s rc %d  states %u  entries %u  prefixes refused %zu\n", argv[a], rc, info.states, info.entries, refused);
	}
	return bad ? 1 : 0;
}
