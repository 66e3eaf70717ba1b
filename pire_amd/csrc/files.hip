// From a hit list and file boundaries to hits by file on the device (pire_hip_files): grep -c / -l / -L / -H -n.
//
// Every hit pass answers "which lines matched" with an ascending list of line numbers.  Where the lines are those of many
// files laid end to end, a caller wants to know which file a hit belongs to: the matches per file, the files with a match,
// the files without one, and for every hit its file and its line number inside that file.  This unit answers from the hit
// list and the files' line boundaries alone -- bounds[files + 1], non-decreasing, file f = the lines [bounds[f],
// bounds[f + 1]); repeated entries are empty files.  It takes no table and no text (include/pire_hip.h has the formulas).
//
//   bounds    one lane per f in [0, files]: first[f] = how many hits lie in front of bounds[f], a lower bound in the list.
//             The hits of file f are hits[first[f], first[f + 1]).  Work is divided by files.
//   classify  one tile = 1 024 FILES: listed <=> (first[f + 1] != first[f]) != without.  The bits of a wave are one ballot
//             word, kept in scratch; one count per tile.
//   scan      exclusive scan of the tile counts, one block (select.hip's kernel, LaunchTileScan); the total is the file count.
//   scatter   rank of a listed file = tile offset + the popcounts of the waves in front + mbcnt of its own wave's word.
//   locate    one tile = 1 024 HITS, only where the caller asks for the file or the line of every hit.  The tile's first and
//             last hit bound the slice of `bounds` any of its lanes needs: two wave-wide searches, 64 probes a step.  A lane
//             then finds the last f with bounds[f] <= hit inside that slice -- no step at all where the tile lies inside one
//             file, the same two searches in every tile of a file that spans many.  The LAST such f: behind a run of empty
//             files it is the one that holds the line.
//   lines     for the lines forms: out_file_lines[f] = how many lines begin in front of byte file_bytes[f], a lower bound in
//             the split's offsets (line i begins at offsets[i] + i of raw), and which boundaries lie inside a line.
//
// The classify and scatter kernels and the launcher are tile_pass.h's, the wave-wide search and the load of a list entry
// compact.h's (WaveBound, LoadU64), the staging of the file count and list internal.h's HitStage; this unit keeps its
// predicate and what a listed file writes (FilesPass), and the bounds, locate and lines kernels.  Launches on the caller's
// stream: no block waits for another block, no atomics (the same input gives the same bits).  Plain HIP with compiler-placed waits: nothing here keeps data on its way in registers.
// `hits` may have any alignment: an entry is read through a packed type.  A list or bounds that break the preconditions
// give unspecified answers and nothing worse: every index into `hits` is clamped into [0, k), every index into `bounds`
// into [0, files].

#include <hip/hip_runtime.h>

#include <algorithm>

#include "tile_pass.h"

namespace pirehip {

namespace {

// (one tile = 1 024 files, or 1 024 hits)
struct FilesPass {
	const uint64_t* hits;       // [k], any alignment
	const uint64_t* hitCount;   // nullable: k = hitCap
	uint64_t hitCap;
	const uint64_t* bounds;     // [files + 1]
	uint64_t files;
	uint32_t without;
	uint64_t* first;            // [files + 1]: the caller's, or scratch
	uint64_t* outHits;          // nullable: the list itself, for a caller whose list lives in scratch
	uint64_t* outHitFile;       // nullable
	uint64_t* outHitLine;       // nullable
	uint64_t outCap;            // entries of the three arrays above
	uint64_t* outFiles;
	uint32_t hitTiles;

	// listed: the file has hits, or -- `without` -- has none
	__device__ __forceinline__ bool Selected(uint64_t f) const { return (first[f + 1] != first[f]) != (without != 0); }
	__device__ __forceinline__ void Write(uint64_t rank, uint64_t f) const { outFiles[rank] = f; }
};

__device__ __forceinline__ uint64_t HitsInList(const FilesPass& p)
{
	return std::min(p.hitCount ? *p.hitCount : p.hitCap, p.hitCap);
}

__global__ __launch_bounds__(kBlockThreads) void FilesBoundsKernel(FilesPass p)
{
	const uint64_t k = HitsInList(p);
	for (uint64_t f = uint64_t(blockIdx.x) * kBlockThreads + threadIdx.x; f <= p.files; f += uint64_t(gridDim.x) * kBlockThreads) {
		const uint64_t x = p.bounds[f];
		uint64_t lo = 0, hi = k;   // how many hits are < x; every probe inside [0, k)
		while (lo < hi) {
			const uint64_t mid = lo + (hi - lo) / 2;
			if (LoadU64(p.hits, mid) < x)
				lo = mid + 1;
			else
				hi = mid;
		}
		p.first[f] = lo;
	}
}

// files > 0
__global__ __launch_bounds__(kBlockThreads) void FilesLocateKernel(FilesPass p)
{
	__shared__ uint64_t slice[2];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t k = HitsInList(p);
	for (uint32_t tile = blockIdx.x; tile < p.hitTiles; tile += gridDim.x) {
		const uint64_t t0 = uint64_t(tile) * kBlockThreads;
		if (t0 >= k)   // (the whole block, and every tile it would take behind this one)
			break;
		const uint64_t t1 = std::min(t0 + kBlockThreads, k);
		// the files of the tile's first and of its last hit: the last f with bounds[f] <= hit, inside [0, files)
		if (wave < 2) {
			const uint64_t c = WaveBound<true>(p.bounds, p.files + 1, LoadU64(p.hits, wave ? t1 - 1 : t0));
			if (lane == 0)
				slice[wave] = std::min(c ? c - 1 : 0, p.files - 1);
		}
		__syncthreads();
		const uint64_t fLo = slice[0], fHi = std::max(slice[1], fLo);
		const uint64_t j = t0 + threadIdx.x;
		if (j < t1 && j < p.outCap) {
			const uint64_t h = LoadU64(p.hits, j);
			uint64_t lo = fLo, hi = fHi;   // the last f in [fLo, fHi] with bounds[f] <= h; every probe inside (fLo, fHi]
			while (lo < hi) {
				const uint64_t mid = lo + (hi - lo + 1) / 2;
				if (p.bounds[mid] <= h)
					lo = mid;
				else
					hi = mid - 1;
			}
			if (p.outHits)
				p.outHits[j] = h;
			if (p.outHitFile)
				p.outHitFile[j] = lo;
			if (p.outHitLine)
				p.outHitLine[j] = h - p.bounds[lo];
		}
		__syncthreads();   // (the next tile writes slice again)
	}
}

struct FileLinesParams {
	const uint64_t* offsets;     // [n + 1] of the split: line i begins at offsets[i] + i of raw
	uint64_t n;
	const uint64_t* fileBytes;   // [files + 1]
	uint64_t files;
	const uint8_t* raw;
	uint64_t size;
	uint32_t delim;
	uint64_t* outLines;          // [files + 1]
	uint32_t* straddles;         // [tiles] boundaries inside a line per tile
	uint32_t tiles;              // of files + 1 entries
};

__global__ __launch_bounds__(kBlockThreads) void FileLinesKernel(FileLinesParams p)
{
	__shared__ uint32_t waveCount[kBlockWaves];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint32_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
		const uint64_t f = uint64_t(tile) * kBlockThreads + threadIdx.x;
		bool inside = false;
		if (f <= p.files) {
			const uint64_t x = p.fileBytes[f];
			uint64_t lo = 0, hi = p.n;   // how many lines begin in front of byte x; every probe inside [0, n)
			while (lo < hi) {
				const uint64_t mid = lo + (hi - lo) / 2;
				if (p.offsets[mid] + mid < x)
					lo = mid + 1;
				else
					hi = mid;
			}
			p.outLines[f] = lo;
			inside = f >= 1 && f < p.files && x > 0 && x < p.size && p.raw[x - 1] != p.delim;
		}
		const uint64_t ballot = __ballot(inside);
		if (lane == 0)
			waveCount[wave] = uint32_t(__popcll(ballot));
		__syncthreads();
		if (threadIdx.x == 0) {
			uint32_t sum = 0;
			for (uint32_t w = 0; w < kBlockWaves; ++w)
				sum += waveCount[w];
			p.straddles[tile] = sum;
		}
		__syncthreads();
	}
}

int Refuse(const char* who, const char* what)
{
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

}  // namespace

int LaunchFiles(const uint64_t* hits, const uint64_t* hitCount, uint64_t hitCap, const uint64_t* bounds, uint64_t files, uint32_t fileMode,
                uint64_t* outFileFirst, uint64_t* outHits, uint64_t* outHitFile, uint64_t* outHitLine, uint64_t outCap, uint64_t* outFiles,
                uint64_t fileCap, uint64_t* outFileCount, hipStream_t stream)
{
	if (files == 0) {
		hipError_t e = hipMemsetAsync(outFileCount, 0, 8, stream);
		if (e == hipSuccess && outFileFirst)
			e = hipMemsetAsync(outFileFirst, 0, 8, stream);
		return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemsetAsync(file count)");
	}
	TilePass t(stream);
	StreamScratch ownFirst(stream);
	const int rc = t.Front("pire_hip_files", "hipMallocAsync(files scratch)", files, outFileCount);
	if (rc || !t.s.tiles)
		return rc;
	FilesPass p;
	if (!outFileFirst) {
		if (int rc2 = ownFirst.Alloc((size_t(files) + 1) * 8, "hipMallocAsync(file first)"))
			return rc2;
		outFileFirst = ownFirst.as<uint64_t>();
	}
	p.hits = hits;
	p.hitCount = hitCount;
	p.hitCap = hitCap;
	p.bounds = bounds;
	p.files = files;
	p.without = fileMode & PIRE_HIP_FILES_WITHOUT;
	p.first = outFileFirst;
	p.outHits = outHits;
	p.outHitFile = outHitFile;
	p.outHitLine = outHitLine;
	p.outCap = std::min(outCap, hitCap);
	p.outFiles = outFiles;
	p.hitTiles = uint32_t((p.outCap + kBlockThreads - 1) / kBlockThreads);
	const dim3 block(kBlockThreads);
	hipLaunchKernelGGL(FilesBoundsKernel, dim3(std::min(uint32_t(files / kBlockThreads) + 1, kTileMaxBlocks)), block, 0, stream, p);
	t.Classify(p, files);
	t.Scan(outFileCount);
	t.Scatter(p, outFiles ? fileCap : 0);
	if (p.hitTiles && (outHits || outHitFile || outHitLine))
		hipLaunchKernelGGL(FilesLocateKernel, dim3(std::min(p.hitTiles, kTileMaxBlocks)), block, 0, stream, p);
	return t.Done("files launch");
}

int LaunchFileLines(const uint64_t* offsets, uint64_t n, const uint64_t* fileBytes, uint64_t files, const void* raw, uint64_t size,
                    uint32_t delim, uint64_t* outFileLines, uint64_t* outStraddles, hipStream_t stream)
{
	if (files == 0) {   // (no boundaries to read)
		hipError_t e = hipMemsetAsync(outStraddles, 0, 8, stream);
		if (e == hipSuccess)
			e = hipMemsetAsync(outFileLines, 0, 8, stream);
		return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "hipMemsetAsync(file lines)");
	}
	FileLinesParams p;
	StreamScratch counts(stream);
	p.tiles = uint32_t(files / kBlockThreads) + 1;   // files + 1 entries
	if (int rc = counts.Alloc(size_t(p.tiles) * 4, "hipMallocAsync(file lines scratch)"))
		return rc;
	p.offsets = offsets;
	p.n = n;
	p.fileBytes = fileBytes;
	p.files = files;
	p.raw = static_cast<const uint8_t*>(raw);
	p.size = size;
	p.delim = delim;
	p.outLines = outFileLines;
	p.straddles = counts.as<uint32_t>();
	hipLaunchKernelGGL(FileLinesKernel, dim3(std::min(p.tiles, kTileMaxBlocks)), dim3(kBlockThreads), 0, stream, p);
	LaunchTileScan(p.straddles, 1, p.tiles, outStraddles, stream);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? PIRE_HIP_OK : HipFail(e, "file lines launch");
}

int FilesArgsInvalid(const char* who, bool haveBounds, const char* boundsName, uint64_t files, uint32_t fileMode, const FilesOut& o)
{
	std::string what = !o.outFileCount               ? "null out_file_count"
	                   : files && !haveBounds        ? std::string("files > 0 with null ") + boundsName
	                   : o.fileCap && !o.outFiles    ? "file_cap > 0 with null out_files"
	                   : fileMode > 1                ? "unknown file_mode"
	                   : files >= (1ull << 32)       ? "2^32 files or more in one call"
	                                                 : "";
	if (what.empty())
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

int FilesBoundsInvalid(const char* who, const char* boundsName, const uint64_t* bounds, uint64_t files, uint64_t total, const char* totalName)
{
	std::string what;
	if (files == 0)
		what = total ? std::string("files == 0 with ") + totalName + " > 0" : "";
	else if (bounds[0] != 0)
		what = std::string(boundsName) + "[0] != 0";
	else if (bounds[files] != total)
		what = std::string(boundsName) + "[files] != " + totalName;
	else
		for (uint64_t f = 0; f < files && what.empty(); ++f)
			if (bounds[f] > bounds[f + 1])
				what = std::string(boundsName) + " must be non-decreasing";
	if (what.empty())
		return PIRE_HIP_OK;
	SetError(std::string(who) + ": " + what);
	return PIRE_HIP_EINVAL;
}

}  // namespace pirehip

using namespace pirehip;

extern "C" int pire_hip_files(const uint64_t* hits, const uint64_t* hit_count, uint64_t hit_cap, uint64_t n, const uint64_t* bounds,
                              uint64_t files, uint32_t file_mode, uint32_t flags, uint64_t* out_file_first, uint64_t* out_hit_file,
                              uint64_t* out_hit_line, uint64_t* out_files, uint64_t file_cap, uint64_t* out_file_count, void* streamPtr)
try {
	const char* who = "pire_hip_files";
	const FilesOut o = {out_files, file_cap, out_file_count};
	if (int rc = FilesArgsInvalid(who, bounds != nullptr, "bounds", files, file_mode, o))
		return rc;
	if (hit_cap && !hits)
		return Refuse(who, "hit_cap > 0 with null hits");
	if (files == 0 && n)
		return Refuse(who, "files == 0 with n > 0");
	if (n >= (1ull << 32))
		return Refuse(who, "2^32 lines or more in one call");
	if (hit_cap >= (1ull << 32))
		return Refuse(who, "2^32 hits or more in one call");
	hipStream_t stream = static_cast<hipStream_t>(streamPtr);
	if (flags & PIRE_HIP_RUN_ON_DEVICE)
		return LaunchFiles(hits, hit_count, hit_cap, bounds, files, file_mode, out_file_first, nullptr, out_hit_file, out_hit_line, hit_cap,
		                   out_files, file_cap, out_file_count, stream);
	// host pointers: the list and the bounds are looked at, staged in, the kernels, staged out -- the file list only as far as
	// it was written
	const uint64_t k = std::min(hit_count ? *hit_count : hit_cap, hit_cap);
	if (int rc = ContextHitsInvalid(who, hits, k, n))
		return rc;
	if (int rc = FilesBoundsInvalid(who, "bounds", bounds, files, n, "n"))
		return rc;
	if (files == 0) {
		*out_file_count = 0;
		if (out_file_first)
			out_file_first[0] = 0;
		return PIRE_HIP_OK;
	}
	BatchIO io(stream, false);
	const uint8_t* dHits = nullptr;
	const uint64_t* dBounds = nullptr;
	HitStage list(false, out_file_count, "hipMemcpy(files)");   // `files` files: no list is staged longer
	uint64_t *dFirst = nullptr, *dHitFile = nullptr, *dHitLine = nullptr, *dFiles = nullptr;
	int rc;
	if (k)
		if ((rc = io.In(reinterpret_cast<const uint8_t*>(hits), size_t(k) * 8, &dHits)))
			return rc;
	if ((rc = io.In(bounds, size_t(files) + 1, &dBounds)) || (rc = list.Count(io, file_cap, files)))
		return rc;
	if (out_file_first)
		if ((rc = io.Result(out_file_first, size_t(files) + 1, size_t(files) + 1, &dFirst)))
			return rc;
	if (out_hit_file && k)
		if ((rc = io.Result(out_hit_file, size_t(k), size_t(k), &dHitFile)))
			return rc;
	if (out_hit_line && k)
		if ((rc = io.Result(out_hit_line, size_t(k), size_t(k), &dHitLine)))
			return rc;
	if ((rc = list.List(io, out_files, 1, &dFiles)) || (rc = io.Ready()))
		return rc;
	if ((rc = LaunchFiles(reinterpret_cast<const uint64_t*>(dHits), nullptr, k, dBounds, files, file_mode, dFirst, nullptr, dHitFile, dHitLine, k,
	                      dFiles, list.cap, list.dCount, stream)))
		return rc;
	if ((rc = io.Finish()))
		return rc;
	return list.Back();
} catch (...) {
	return pirehip::HandleException();   // an exception must not unwind through the C ABI
}
