/*
 * batch_runner.hpp -- header-only C++ shim that keeps the Pire::Scanner / Pire::Runner vocabulary on top of the
 * C ABI of libpire_hip.so (include/pire_hip.h).  This is the binding a Pire maintainer would add:
 * the reference has no FFI on this path, it is a compile-time template concept (pire/run.h:50-57, 271-275,
 * 365-392), so the drop-in is a class with the same fluent surface, batched over N strings:
 *
 *     Pire::Scanner sc = ...;                                  // built by the reference, on the host, unchanged
 *     Pire::Hip::BatchRunner<Pire::Scanner> run(sc);           // Save() -> pire_hip_table_create()
 *     run.Begin().Run(text, offsets, n).End();                 // == for each i: Runner(sc).Begin().Run(..).End()
 *     const auto& states = run.States();                       // std::vector<Pire::Scanner::State>
 *     bool ok = sc.Final(states[i]);                           // every Scanner accessor keeps working
 *     auto ids = sc.AcceptedRegexps(states[i]);
 *
 * It compiles against the unmodified reference headers (<pire/pire.h>); nothing in it re-implements the walk: the
 * states come back from the GPU as StateIndex values and are turned into Scanner::State (a row address inside the
 * host scanner) with public API only -- Initialize(), StateIndex(), LettersCount(), sizeof(ScannerRowHeader),
 * Transition (pire/scanners/multi.h:161, 281-284, 140, 119, 99, 347).
 *
 * Errors: the C ABI's negative codes are re-thrown as Pire::Error (pire/stub/stl.h:213-217), the reference's own
 * exception type for this library.
 *
 * The map.  What the runners have in common has one definition each:
 *     SavedBlob()       a scanner's Save() form, for every *_table_create            Table, CountedBatchRunner's two, Capture, Slow
 *     OwnedStrings      a std::vector<ystring> as one text and offsets; OffsetsOr(): the {0} that stands in for the offsets of no
 *                       strings                                                      every Run(vector), every call that takes offsets
 *     GrowAndRetry()    one call at a first capacity, one more where the answer did not fit       BatchRunner's lines, text and route
 *                       forms, CountedBatchRunner, CaptureBatchRunner, SlowBatchRunner, AffixBatchRunner
 *     Table             the device table, State <-> StateIndex (ToStates), Regexps()              BatchRunner, Multi-, Pair-, AffixBatchRunner
 *     CountedBatchRunner   all of HalfFinalBatchRunner and CountingBatchRunner but their table and their three C calls
 *     LineMatcher       easy.h's choice between Scanner and SlowScanner, one lines surface over BatchRunner and SlowBatchRunner
 *     LineContext       a Context(before, after) and what was fetched for it                      BatchRunner, SlowBatchRunner
 *     LineFiles         a Files(fileBytes) and what was fetched for it                            BatchRunner, SlowBatchRunner
 *     LineQuery, Truth  several scanners over the lines of one buffer and a boolean function of what they match; tables of its own
 *     Substitution      the matches of a MatchFinder replaced in a buffer of lines, the rest kept; tables of its own
 * Which C calls these make, in which order and with which arguments, is recorded: tests/cpp/shim_calls_test.cpp,
 * tests/cpp/shim_calls.expected.txt.
 */
#ifndef PIRE_HIP_BATCH_RUNNER_HPP
#define PIRE_HIP_BATCH_RUNNER_HPP

#include <algorithm>
#include <cstdint>
#include <sstream>
#include <string>
#include <vector>

#include <pire/pire.h>

#include "../pire_hip.h"

namespace Pire {
namespace Hip {

inline void Check(int rc)
{
	if (rc < 0)
		throw Pire::Error(std::string("pire_hip: ") + pire_hip_last_error());
}

/* The PUBLIC hand-off of every scanner: its Save() form (Scanner::Save, multi.h:307, 557-573; NonrelocScanner saves as
 * Relocatable, 604-608; SimpleScanner, scanner_io.cpp:35-49; SlowScanner, 71-111; LoadedScanner, 172-189 / count.cpp:1009-1018) */
template <class AnyScanner>
std::string SavedBlob(const AnyScanner& sc)
{
	std::ostringstream out;
	sc.Save(&out);
	return out.str();
}

/* A caller's std::vector<ystring> as the C calls take strings: one text, n + 1 offsets. */
class OwnedStrings {
public:
	void Assign(const std::vector<ystring>& strings)
	{
		m_text.clear();
		m_offsets.assign(1, 0);
		for (size_t i = 0; i < strings.size(); ++i) {
			m_text.append(strings[i]);
			m_offsets.push_back(m_text.size());
		}
	}
	const char* Text() const { return m_text.data(); }
	const uint64_t* Offsets() const { return m_offsets.data(); }

	/* The offsets of a batch of host strings: with no strings the caller need not have any. */
	static const uint64_t* OffsetsOr(const uint64_t* offsets, size_t n)
	{
		static const uint64_t kNoOffsets[1] = {0};
		return n ? offsets : kNoOffsets;
	}

private:
	ystring m_text;
	std::vector<uint64_t> m_offsets;
};

/*
 * One call with room for `first` answers, and a second one where there were more: call(cap) makes the call with room for cap
 * and returns how many it needed (a call with that much room fits).  Returns the capacity of the call that fit.
 */
template <class Call>
size_t GrowAndRetry(size_t first, Call call)
{
	for (size_t cap = first;;) {
		const size_t needed = call(cap);
		if (needed <= cap)
			return cap;
		cap = needed;
	}
}

/*
 * The lines around the hits of a RunLines(): grep -A / -B / -C on the device (include/pire_hip.h, "the lines around a match").
 * What BatchRunner and SlowBatchRunner keep of a Context(before, after): the request, and what was fetched for it -- lazily,
 * under a Has / Stale scheme of its own: the lists with the first accessor that asks (the select form), the text with
 * ContextText() (the gather form, a call of its own as HitText() is).  The runner makes the C call: call(Call) fills in its
 * table, buffer, flags and selection.
 */
class LineContext {
public:
	struct Call {
		uint64_t before, after;
		uint64_t* lineCount;
		uint64_t* lines;       // null in the gather form
		uint8_t* flags;
		uint64_t* spans;
		uint64_t cap;
		uint64_t *selCount, *groupCount, *hitCount;
		bool gather;
		uint32_t tail;
		char* text;
		uint64_t textCap;
		uint64_t* offsets;
		uint64_t* bytes;
	};
	LineContext() : m_before(0), m_after(0), m_asked(false), m_current(0), m_textTail('\n'), m_lineCount(0), m_selCount(0), m_groupCount(0), m_hitCount(0) {}
	void Ask(uint64_t before, uint64_t after)
	{
		m_before = before, m_after = after, m_asked = true;
		Stale(kLists | kText);
	}
	void NewSelection() { Stale(kLists | kText); }   // the request stays
	void NewBatch()                                  // the request goes with the batch it was made for
	{
		m_asked = false;
		Stale(kLists | kText);
	}
	/* One call with room for a selected line per 64 bytes of the buffer, and a second one where there are more */
	template <class Fn>
	void FetchLists(const char* what, size_t len, Fn call)
	{
		Need(what);
		if (Has(kLists))
			return;
		GrowAndRetry(len / 64 + 1024, [&](size_t cap) {
			m_lines.resize(cap);
			m_flags.resize(cap);
			m_spans.resize(cap * 2);
			const Call c = {m_before, m_after, &m_lineCount, m_lines.data(), m_flags.data(), m_spans.data(), cap, &m_selCount, &m_groupCount,
			                &m_hitCount, false, 0, nullptr, 0, nullptr, nullptr};
			call(c);
			return size_t(m_selCount);
		});
		m_lines.resize(m_selCount);
		m_flags.resize(m_selCount);
		m_spans.resize(m_selCount * 2);
		m_current |= kLists;
	}
	/* The selected lines as bytes; room for every byte they can have, and for the lines that are known, or else FetchLists()'s */
	template <class Fn>
	void FetchText(const char* what, size_t len, char tail, Fn call)
	{
		Need(what);
		if (Has(kText) && m_textTail == tail)
			return;
		uint64_t count = 0, groups = 0, hits = 0, bytes = 0;
		GrowAndRetry(Has(kLists) ? size_t(m_selCount) : len / 64 + 1024, [&](size_t cap) {
			m_textOffsets.resize(cap + 1);
			m_text.resize(len + cap + 1);
			const Call c = {m_before, m_after, &m_lineCount, nullptr, nullptr, nullptr, cap, &count, &groups, &hits, true, uint8_t(tail),
			                &m_text[0], m_text.size(), m_textOffsets.data(), &bytes};
			call(c);
			return size_t(count);   // (the text has room for the whole buffer and a tail per line: where the lines fit, the bytes do)
		});
		m_text.resize(bytes);
		m_textOffsets.resize(count + 1);
		m_textTail = tail;
		m_current |= kText;
	}
	bool HasText() const { return Has(kText); }
	const std::vector<uint64_t>& Lines() const { return m_lines; }
	const std::vector<uint8_t>& Flags() const { return m_flags; }
	const std::vector<uint64_t>& Spans() const { return m_spans; }
	uint64_t GroupCount() const { return m_groupCount; }
	const std::string& Text() const { return m_text; }
	const std::vector<uint64_t>& TextOffsets() const { return m_textOffsets; }

private:
	enum Result { kLists = 1 << 0, kText = 1 << 1 };   // m_lines .. m_hitCount / m_text, m_textOffsets are the request's, with the tail m_textTail
	bool Has(unsigned results) const { return (m_current & results) == results; }
	void Stale(unsigned results) { m_current &= ~results; }
	void Need(const char* what) const
	{
		if (!m_asked)
			throw Pire::Error(std::string("pire_hip: ") + what + " follows Context()");
	}
	uint64_t m_before, m_after;
	bool m_asked;
	unsigned m_current;
	char m_textTail;
	uint64_t m_lineCount, m_selCount, m_groupCount, m_hitCount;
	std::vector<uint64_t> m_lines, m_spans, m_textOffsets;
	std::vector<uint8_t> m_flags;
	std::string m_text;
};

/*
 * The hits of a RunLines() by file: grep -c / -l / -L / -H -n over many files laid end to end in one buffer (include/pire_hip.h,
 * "hits by file").  What BatchRunner and SlowBatchRunner keep of a Files(fileBytes): the request, and what was fetched for it
 * -- lazily, as LineContext does: the lists with the first accessor that asks, the files WITHOUT a hit with a call of their
 * own (the other file_mode, no room for hits).  The runner makes the C call: call(Call) fills in its table, buffer, flags and
 * selection.
 */
class LineFiles {
public:
	struct Call {
		const uint64_t* fileBytes;
		uint64_t files;
		uint32_t fileMode;
		uint64_t* lineCount;
		uint64_t *hits, *spans, *hitFile, *hitLine;
		uint64_t cap;
		uint64_t* hitCount;
		uint64_t *fileLines, *fileFirst, *outFiles;
		uint64_t fileCap;
		uint64_t *fileCount, *straddles;
	};
	LineFiles() : m_asked(false), m_current(0), m_lineCount(0), m_hitCount(0), m_straddles(0) {}
	void Ask(const std::vector<uint64_t>& fileBytes)
	{
		m_fileBytes = fileBytes, m_asked = true;
		Stale(kLists | kWithout);
	}
	void NewSelection() { Stale(kLists | kWithout); }   // the request stays
	void NewBatch()                                     // the request goes with the batch it was made for
	{
		m_asked = false;
		Stale(kLists | kWithout);
	}
	/* One call with room for a hit per 64 bytes of the buffer, and a second one where there are more */
	template <class Fn>
	void FetchLists(const char* what, size_t len, Fn call)
	{
		Need(what);
		if (Has(kLists))
			return;
		const size_t files = Files();
		uint64_t listed = 0;
		m_fileLines.assign(files + 1, 0);
		m_first.assign(files + 1, 0);
		m_with.assign(files, 0);
		GrowAndRetry(len / 64 + 1024, [&](size_t cap) {
			m_hits.resize(cap);
			m_hitFile.resize(cap);
			m_hitLine.resize(cap);
			const Call c = {Bytes(), files, 0, &m_lineCount, m_hits.data(), nullptr, m_hitFile.data(), m_hitLine.data(), cap, &m_hitCount,
			                m_fileLines.data(), m_first.data(), files ? m_with.data() : nullptr, files, &listed, &m_straddles};
			call(c);
			return size_t(m_hitCount);
		});
		m_hits.resize(m_hitCount);
		m_hitFile.resize(m_hitCount);
		m_hitLine.resize(m_hitCount);
		m_with.resize(listed);
		m_counts.resize(files);
		for (size_t f = 0; f < files; ++f)
			m_counts[f] = m_first[f + 1] - m_first[f];
		m_current |= kLists;
	}
	/* The files without a hit: the other file_mode, no room for hits */
	template <class Fn>
	void FetchWithout(const char* what, Fn call)
	{
		Need(what);
		if (Has(kWithout))
			return;
		const size_t files = Files();
		uint64_t lines = 0, hits = 0, listed = 0, straddles = 0;
		m_without.assign(files, 0);
		const Call c = {Bytes(), files, PIRE_HIP_FILES_WITHOUT, &lines, nullptr, nullptr, nullptr, nullptr, 0, &hits, nullptr, nullptr,
		                files ? m_without.data() : nullptr, files, &listed, &straddles};
		call(c);
		m_without.resize(listed);
		m_current |= kWithout;
	}
	const std::vector<uint64_t>& Counts() const { return m_counts; }
	const std::vector<uint64_t>& With() const { return m_with; }
	const std::vector<uint64_t>& Without() const { return m_without; }
	const std::vector<uint64_t>& HitFile() const { return m_hitFile; }
	const std::vector<uint64_t>& HitLine() const { return m_hitLine; }
	const std::vector<uint64_t>& FileLines() const { return m_fileLines; }
	uint64_t Straddles() const { return m_straddles; }

private:
	enum Result { kLists = 1 << 0, kWithout = 1 << 1 };
	bool Has(unsigned results) const { return (m_current & results) == results; }
	void Stale(unsigned results) { m_current &= ~results; }
	void Need(const char* what) const
	{
		if (!m_asked)
			throw Pire::Error(std::string("pire_hip: ") + what + " follows Files()");
	}
	size_t Files() const { return m_fileBytes.empty() ? 0 : m_fileBytes.size() - 1; }
	const uint64_t* Bytes() const { return m_fileBytes.empty() ? nullptr : m_fileBytes.data(); }
	bool m_asked;
	unsigned m_current;
	uint64_t m_lineCount, m_hitCount, m_straddles;
	std::vector<uint64_t> m_fileBytes, m_hits, m_hitFile, m_hitLine, m_fileLines, m_first, m_counts, m_with, m_without;
};

/*
 * Many buffers as the one a Files() request takes: the files laid end to end, the delimiter appended behind a non-empty file
 * that does not end in it -- so no boundary lies inside a line and Straddles() is 0 for what this builds.  Host only.
 *     FileSet set;   set.Add("a.log", data, size);   ...   run.RunLines(set.Raw().data(), set.Raw().size()).Files(set.Bytes());
 */
class FileSet {
public:
	explicit FileSet(char delim = '\n') : m_delim(delim), m_bytes(1, 0) {}
	void Add(const std::string& name, const char* data, size_t size)
	{
		m_names.push_back(name);
		if (size) {
			m_raw.append(data, size);
			if (data[size - 1] != m_delim)
				m_raw.push_back(m_delim);
		}
		m_bytes.push_back(m_raw.size());
	}
	const std::string& Raw() const { return m_raw; }
	const std::vector<uint64_t>& Bytes() const { return m_bytes; }   // [Size() + 1]: file f is Raw()[Bytes()[f], Bytes()[f + 1])
	const std::string& Name(size_t f) const { return m_names[f]; }
	size_t Size() const { return m_names.size(); }

private:
	char m_delim;
	std::string m_raw;
	std::vector<uint64_t> m_bytes;
	std::vector<std::string> m_names;
};

/* Bytes between the State values of consecutive StateIndex numbers, from public API only. */
template <class Scanner>
struct RowGeometry {
	static size_t Stride(const Scanner& sc)
	{
		typedef typename Scanner::Transition Tr;
		const size_t header = sizeof(typename Scanner::ScannerRowHeader) / sizeof(Tr);           // HEADER_SIZE, multi.h:349
		const size_t align = sizeof(Pire::Impl::MaxSizeWord) / sizeof(Tr);
		const size_t row = (sc.LettersCount() + header + align - 1) / align * align;             // RowSize(), multi.h:347
		return row * sizeof(Tr);
	}
};
template <>
struct RowGeometry<Pire::SimpleScanner> {
	static size_t Stride(const Pire::SimpleScanner&)
	{
		return (Pire::MaxChar + 1) * sizeof(Pire::SimpleScanner::Transition);                    // STATE_ROW_SIZE, simple.h:43
	}
};

/* A device-side copy of a compiled scanner.  Immutable, shareable between threads, like the scanner itself. */
template <class Scanner>
class Table {
public:
	explicit Table(const Scanner& sc)
	    : m_table(nullptr)
	{
		if (pire_hip_abi_version() != PIRE_HIP_ABI_VERSION)   // structs of this header vs. the loaded library's: refuse, do not guess
			throw Pire::Error("pire_hip: libpire_hip.so was built with another ABI version than this header");
		const std::string blob = SavedBlob(sc);
		Check(pire_hip_table_create(blob.data(), blob.size(), &m_table));

		// State <-> StateIndex geometry of THIS host scanner, public API only
		m_stride = RowGeometry<Scanner>::Stride(sc);
		typename Scanner::State init;
		sc.Initialize(init);
		m_base = init - sc.StateIndex(init) * m_stride;
	}
	~Table() { pire_hip_table_destroy(m_table); }

	pire_hip_table* Handle() const { return m_table; }

	/* Which states have rows in LDS is a performance choice the table makes from a byte model of text and then corrects
	 * from what the scans really visit -- by itself (pire_hip_config.auto_adapt = 0, the default: a worker thread re-ranks a
	 * copy of the table and a later launch swaps it in; no call is made to wait), or here, explicitly, after a representative
	 * batch.  Results never depend on it.  Returns the number of rows that entered the dense set.  May run while other
	 * threads scan with this table (it joins a running worker first). */
	unsigned Adapt()
	{
		uint32_t changed = 0;
		Check(pire_hip_table_adapt(m_table, &changed));
		return changed;
	}
	/* The automatic form off (true) or on (false) for the whole library; see pire_hip_config. */
	static void FreezeRanking(bool frozen)
	{
		pire_hip_config c;
		c.size = sizeof(c);
		Check(pire_hip_config_get(&c));
		c.auto_adapt = frozen ? 1 : 0;
		Check(pire_hip_config_set(&c));
	}
	typename Scanner::State ToState(uint32_t idx) const { return m_base + size_t(idx) * m_stride; }
	uint32_t ToIndex(typename Scanner::State st) const { return uint32_t((st - m_base) / m_stride); }
	/* What a scan leaves per string, as the reference has it: StateIndex -> State */
	void ToStates(const std::vector<uint32_t>& idx, std::vector<typename Scanner::State>& states) const
	{
		states.resize(idx.size());
		for (size_t i = 0; i < idx.size(); ++i)
			states[i] = ToState(idx[i]);
	}
	/* RegexpsCount() as the library has it */
	size_t Regexps() const
	{
		pire_hip_table_info info;
		Check(pire_hip_table_get_info(m_table, &info));
		return size_t(info.regexps);
	}

private:
	Table(const Table&);
	Table& operator=(const Table&);
	pire_hip_table* m_table;
	size_t m_base, m_stride;
};

/* A device buffer owned by the shim (grown on demand, freed with its owner). */
class DeviceBuffer {
public:
	DeviceBuffer() : m_ptr(nullptr), m_bytes(0) {}
	~DeviceBuffer() { pire_hip_device_free(m_ptr); }
	void* Reserve(size_t bytes)
	{
		if (bytes > m_bytes) {
			pire_hip_device_free(m_ptr);
			m_ptr = nullptr;
			m_bytes = 0;
			Check(pire_hip_device_alloc(bytes, &m_ptr));
			m_bytes = bytes;
		}
		return m_ptr;
	}
	void* Get() const { return m_ptr; }

private:
	DeviceBuffer(const DeviceBuffer&);
	DeviceBuffer& operator=(const DeviceBuffer&);
	void* m_ptr;
	size_t m_bytes;
};

/*
 * Batched twin of Pire::RunHelper (run.h:365-386).
 *
 * Two ways to hand the text over:
 *   Run(text, offsets, n)                     host pointers: the library moves the text over PCIe chunk by chunk,
 *                                             overlapped with the scan (PCIe bound, ~50 GB/s);
 *   RunDevice(text, offsets, n, stream)       DEVICE pointers: the text is already resident in HBM (a corpus that was
 *   RunDeviceStrided(text, n, len, stride, ..) loaded once, the output of another kernel); the scan runs at the speed
 *                                             of the C ABI (TB/s).  Results stay on the device until asked for:
 *                                             MatchCounts() moves 8 * (regexps + 2) bytes, States()/Finals() 5 bytes
 *                                             per string; DeviceStateIndices()/DeviceFinals() move nothing.
 */
template <class Scanner>
class BatchRunner {
public:
	typedef typename Scanner::State State;

	explicit BatchRunner(const Scanner& sc)
	    : m_own(new Table<Scanner>(sc)), m_table(m_own) { Reset(); }
	/* Re-use one device table for many batches. */
	explicit BatchRunner(const Table<Scanner>& table)
	    : m_own(nullptr), m_table(&table) { Reset(); }
	~BatchRunner() { delete m_own; }

	/* RunHelper(sc, st): resume every string from a previously returned state (run.h:368, 391-392). */
	BatchRunner& From(const std::vector<State>& states)
	{
		m_init.resize(states.size());
		for (size_t i = 0; i < states.size(); ++i)
			m_init[i] = m_table->ToIndex(states[i]);
		return *this;
	}

	BatchRunner& Begin() { m_flags |= PIRE_HIP_RUN_BEGIN; return *this; }     // run.h:375
	BatchRunner& End() { m_flags |= PIRE_HIP_RUN_END; return *this; }         // run.h:376

	/* Run(begin,end) for n strings: string i = text[offsets[i], offsets[i+1]).  Host pointers. */
	BatchRunner& Run(const char* text, const uint64_t* offsets, size_t n) { return SetBatch(kHostOffsets, text, offsets, n); }

	/* The same with DEVICE pointers (text and offsets resident in HBM); `stream` is a hipStream_t or null. */
	BatchRunner& RunDevice(const void* deviceText, const uint64_t* deviceOffsets, size_t n, void* stream = nullptr)
	{
		m_stream = stream;
		return SetBatch(kDeviceOffsets, deviceText, deviceOffsets, n);
	}

	/* Device-resident fixed-length records: string i = text[i * stride, i * stride + len). */
	BatchRunner& RunDeviceStrided(const void* deviceText, size_t n, size_t len, size_t stride, void* stream = nullptr)
	{
		m_stream = stream;
		return SetBatch(kDeviceStrided, deviceText, nullptr, n, len, stride);
	}

	/* Convenience: a vector of strings (copied into one buffer). */
	BatchRunner& Run(const std::vector<ystring>& strings)
	{
		m_ownStrings.Assign(strings);
		return Run(m_ownStrings.Text(), m_ownStrings.Offsets(), strings.size());
	}

	/*
	 * A buffer as it was read -- lines with `delim` between them, host pointer -- cut into lines, scanned and selected on
	 * the device (pire_hip_run_lines_select; getline's semantics: the delimiter is not part of a line, a trailing fragment
	 * is one):
	 *     run.Begin().RunLines(raw, size).End();
	 *     run.HitSpans()    [2 * k], [2 * k + 1]: hit k is raw[begin, end)       run.LineCount()  lines in the buffer
	 *     run.Hits()        the numbers of the selected lines, ascending         run.HitCount() / HitMasks() as after Select()
	 *     run.HitText()     the selected lines back to back, '\n' (or the byte given) behind each: grep's output, gathered on
	 *                       the device (pire_hip_run_lines_gather)       run.HitTextOffsets()  hit k is HitText()[o[k], o[k + 1])
	 * Select({..}) in front of them chooses regexps.  This form has hits only: States() / Finals() / MatchCounts() throw.
	 */
	BatchRunner& RunLines(const char* raw, size_t size, char delim = '\n')
	{
		m_delim = uint8_t(delim);
		return SetBatch(kLines, raw, nullptr, 0, size);
	}
	/*
	 * The same for records: the lines whose COLUMN `field` (from 0, `sep` between the columns) matches -- awk -F'\t' '$3 ~ /re/'
	 * is RunLinesField(raw, size, 2) --, cut, scanned and selected on the device (pire_hip_run_lines_field_select / _gather).
	 * Begin() and End() step the marks around the column, so an anchored pattern anchors to it; rest: the column runs to the end
	 * of the line (cut -f k-).  A line with too few columns is scanned as the empty string.  Hits(), HitSpans() (the WHOLE lines
	 * in raw), HitText() and the rest are RunLines()'s; Route() is not available after this form.
	 */
	BatchRunner& RunLinesField(const char* raw, size_t size, uint32_t field, char sep = '\t', char delim = '\n', bool rest = false)
	{
		m_delim = uint8_t(delim);
		m_sep = uint8_t(sep);
		m_field = field;
		m_fieldMode = rest ? PIRE_HIP_FIELDS_REST : 0;
		return SetBatch(kLinesField, raw, nullptr, 0, size);
	}
	uint64_t LineCount() { FetchHits(); return m_lineCount; }
	const std::vector<uint64_t>& HitSpans() { FetchHits(); return m_hitSpans; }
	/* Fetched lazily, like HitSpans(); the offsets are those of the text fetched last ('\n' where none was).  The text comes from
	 * a call of its own (pire_hip_run_lines_gather: split, scan, select, gather): HitText() after HitSpans() / Hits() scans the
	 * buffer a second time -- ask for the one or the other. */
	const std::string& HitText(char tail = '\n') { FetchHitText(tail); return m_hitText; }
	const std::vector<uint64_t>& HitTextOffsets()
	{
		if (!Has(kHitText))
			FetchHitText('\n');
		return m_hitTextOffsets;
	}

	/*
	 * The hits of RunLines() and the lines around them: grep -A after -B before (pire_hip_run_lines_context_select / _gather).
	 *     run.Begin().RunLines(raw, size).End().Context(2, 2);      Select({..}) in front of it chooses regexps
	 *     run.ContextLines()   the numbers of the selected lines, ascending      run.ContextSpans()  line k is raw[begin, end)
	 *     run.ContextFlags()   PIRE_HIP_CONTEXT_HIT | PIRE_HIP_CONTEXT_GROUP per line     run.ContextGroupCount()  the runs
	 *     run.ContextText()    the lines back to back, '\n' (or the byte given) behind each: grep --no-group-separator's output
	 *     run.ContextTextOffsets()   line k is ContextText()[o[k], o[k + 1])
	 * Fetched lazily; the text is a call of its own, as HitText() is.  A new batch ends the request, a new selection keeps it.
	 * After anything but RunLines() it throws.
	 */
	BatchRunner& Context(uint64_t before, uint64_t after)
	{
		if (m_form != kLines)
			throw Pire::Error("pire_hip: Context() follows RunLines()");
		m_context.Ask(before, after);
		return *this;
	}
	const std::vector<uint64_t>& ContextLines() { FetchContext("ContextLines()"); return m_context.Lines(); }
	const std::vector<uint8_t>& ContextFlags() { FetchContext("ContextFlags()"); return m_context.Flags(); }
	const std::vector<uint64_t>& ContextSpans() { FetchContext("ContextSpans()"); return m_context.Spans(); }
	uint64_t ContextGroupCount() { FetchContext("ContextGroupCount()"); return m_context.GroupCount(); }
	const std::string& ContextText(char tail = '\n') { FetchContextText("ContextText()", tail); return m_context.Text(); }
	const std::vector<uint64_t>& ContextTextOffsets()
	{
		if (!m_context.HasText())
			FetchContextText("ContextTextOffsets()", '\n');
		return m_context.TextOffsets();
	}

	/*
	 * The hits of RunLines() by file, where the buffer is many files laid end to end (pire_hip_run_lines_files_select):
	 * fileBytes[files + 1], from 0 to size, file f = raw[fileBytes[f], fileBytes[f + 1]) -- FileSet builds both.
	 *     run.Begin().RunLines(raw, size).End().Files(set.Bytes());     Select({..}) in front of it chooses regexps
	 *     run.FileHitCounts()     the matches of every file: grep -c          run.FileLines()   [files + 1]: file f is the lines [l[f], l[f + 1])
	 *     run.FilesWithHits()     grep -l        run.FilesWithoutHits()  grep -L (a call of its own)
	 *     run.HitFiles()          the file of every hit, in the order of Hits()       run.HitFileLines()  its line inside that file, from 0
	 *     run.Straddles()         boundaries inside a line: 0 for a FileSet
	 * Fetched lazily.  A new batch ends the request, a new selection keeps it.  After anything but RunLines() it throws.
	 */
	BatchRunner& Files(const std::vector<uint64_t>& fileBytes)
	{
		if (m_form != kLines)
			throw Pire::Error("pire_hip: Files() follows RunLines()");
		m_files.Ask(fileBytes);
		return *this;
	}
	const std::vector<uint64_t>& FileHitCounts() { FetchFiles("FileHitCounts()"); return m_files.Counts(); }
	const std::vector<uint64_t>& FilesWithHits() { FetchFiles("FilesWithHits()"); return m_files.With(); }
	const std::vector<uint64_t>& FilesWithoutHits() { FetchFilesWithout("FilesWithoutHits()"); return m_files.Without(); }
	const std::vector<uint64_t>& HitFiles() { FetchFiles("HitFiles()"); return m_files.HitFile(); }
	const std::vector<uint64_t>& HitFileLines() { FetchFiles("HitFileLines()"); return m_files.HitLine(); }
	const std::vector<uint64_t>& FileLines() { FetchFiles("FileLines()"); return m_files.FileLines(); }
	uint64_t Straddles() { FetchFiles("Straddles()"); return m_files.Straddles(); }

	/* RunHelper::State() per string (run.h:378). */
	const std::vector<State>& States()
	{
		Fetch();
		return m_states;
	}

	/* operator bool of RunHelper per string (run.h:380): Final(State()). */
	const std::vector<char>& Finals()
	{
		Fetch();
		return m_final;
	}

	/* [0] strings ending in a final state, [1] strings scanned, [2+r] strings accepting regexp r. */
	const std::vector<uint64_t>& MatchCounts()
	{
		Execute();
		if (!Has(kCounts)) {
			Check(pire_hip_copy_to_host(m_counts.data(), m_devCounts.Get(), m_counts.size() * 8, m_stream));
			Check(pire_hip_stream_synchronize(m_stream));
			m_current |= kCounts;
		}
		return m_counts;
	}

	/* After RunDevice*: the results where the scan left them -- uint32 StateIndex and uint8 Final per string, device
	 * memory owned by this runner, valid until its next Run*; ordered after the scan on the stream given to RunDevice. */
	const uint32_t* DeviceStateIndices() { Execute(); return static_cast<const uint32_t*>(m_devIdx.Get()); }
	const uint8_t* DeviceFinals() { Execute(); return static_cast<const uint8_t*>(m_devFin.Get()); }

	/*
	 * Which strings matched which regexps, answered on the device (pire_hip_select) -- after a Run*().End():
	 *     run.Begin().Run(text, offsets, n).End().Select();      // the strings that end in a Final state
	 *     run.Select({2, 5});                                    // ... that match regexp 2 or regexp 5
	 *     run.Hits()       ascending indices of the selected strings          run.HitCount()  how many
	 *     run.HitMasks()   MaskWords() words per hit: bit r of the mask <=> r is in AcceptedRegexps(State())
	 * The host loop over States() with one Final / AcceptedRegexps lookup per string gives the same answer in time
	 * proportional to the batch; this one moves 8 * (1 + MaskWords()) bytes per HIT.  After RunDevice*: DeviceHits() /
	 * DeviceHitMasks() / DeviceHitCount() leave them where a consumer on the GPU wants them (ordered on RunDevice's stream).
	 */
	BatchRunner& Select(const std::vector<size_t>& want = std::vector<size_t>())
	{
		m_want.assign(MaskWords(), 0);
		m_haveWant = !want.empty();
		for (size_t i = 0; i < want.size(); ++i)
			if (want[i] < m_want.size() * 64)
				m_want[want[i] / 64] |= uint64_t(1) << (want[i] % 64);
		Stale(kSelection | kHits | kHitText);
		m_context.NewSelection();
		m_files.NewSelection();
		return *this;
	}
	size_t MaskWords() const { return pire_hip_table_mask_words(m_table->Handle()); }
	uint64_t HitCount() { FetchHits(); return m_hitCount; }
	const std::vector<uint64_t>& Hits() { FetchHits(); return m_hits; }
	const std::vector<uint64_t>& HitMasks() { FetchHits(); return m_hitMasks; }
	const uint64_t* DeviceHits() { ExecuteSelect(); return static_cast<const uint64_t*>(m_devHits.Get()); }
	const uint64_t* DeviceHitMasks() { ExecuteSelect(); return static_cast<const uint64_t*>(m_devHitMasks.Get()); }
	const uint64_t* DeviceHitCount() { ExecuteSelect(); return static_cast<const uint64_t*>(m_devHitCount.Get()); }

	/*
	 * One hit list PER REGEXP, answered on the device (pire_hip_route) -- after a Run*().End(), and after RunLines():
	 *     run.Begin().Run(text, offsets, n).End().Route();
	 *     run.RouteCount(r)   how many strings matched regexp r       run.RouteHits(r)  their indices, ascending
	 *     run.Begin().RunLines(raw, size).End().Route();              the same per line of raw, and
	 *     run.RouteSpans(r)   [2 * k], [2 * k + 1]: hit k of regexp r is raw[begin, end)
	 * The host loop over States() with one AcceptedRegexps lookup per string, bucketed by regexp, gives the same answer.
	 * After RunDevice*: DeviceRouteHits() ([RegexpsCount()][RoutePitch()], row r at r * RoutePitch()) and DeviceRouteCounts()
	 * ([RegexpsCount()]) leave them where a consumer on the GPU wants them -- pire_hip_gather takes row r and its count as
	 * they lie (ordered on RunDevice's stream).
	 */
	BatchRunner& Route()
	{
		Stale(kRoute | kRouteRows);
		return *this;
	}
	uint64_t RouteCount(size_t r) { FetchRoute(); return m_routeCounts.at(r); }
	const std::vector<uint64_t>& RouteHits(size_t r) { FetchRoute(); return m_routeHits.at(r); }
	const std::vector<uint64_t>& RouteSpans(size_t r)
	{
		if (!Lines())
			throw Pire::Error("pire_hip: RouteSpans() follows RunLines()");
		FetchRoute();
		return m_routeSpans.at(r);
	}
	const uint64_t* DeviceRouteHits() { ExecuteRoute(); return static_cast<const uint64_t*>(m_devRouteHits.Get()); }
	const uint64_t* DeviceRouteCounts() { ExecuteRoute(); return static_cast<const uint64_t*>(m_devRouteCounts.Get()); }
	size_t RoutePitch() { ExecuteRoute(); return m_routePitch; }

	const Table<Scanner>& GetTable() const { return *m_table; }
	uint32_t Flags() const { return m_flags; }

private:
	/* ---- the batch and what is known of it -------------------------------------------------------------------------------
	 * The batch is one of five forms, set by SetBatch() alone.  What was computed from it is a set of Result bits: a step sets
	 * its bit where it ends, and a bit goes away in two ways.  What the caller does:
	 *     SetBatch()   Run*() of strings: the scan and everything but the selection;  RunLines*(): everything
	 *     Select()     the selection, the hits on the host, the hit text
	 *     Route()      the hit lists per regexp, on the device and on the host
	 * And a step that runs again ends the host copy of what it is about to make anew, with a Stale() of its own:
	 *     Execute()         kStates, kCounts (kCounts is set again at once where the counts came back with the scan)
	 *     ExecuteSelect()   kHits, after RunDevice*(): the hits wait on the device for FetchHits()
	 *     ExecuteRoute()    kRouteRows, after RunDevice*(): the rows wait on the device for FetchRoute()
	 * A result is current while its bit AND the scan's are set -- asked BEFORE the scan is brought up to date, see
	 * SelectionCurrent() --, so a new result is one name in Result and one in the Stale() that ends it. */
	enum Form { kHostOffsets, kDeviceOffsets, kDeviceStrided, kLines, kLinesField };
	enum Result {
		kScan = 1 << 0,        // the scan ran (for the lines forms: a call that scans ran)
		kStates = 1 << 1,      // m_idx / m_fin / m_states / m_final are this scan's
		kCounts = 1 << 2,      // m_counts is
		kSelection = 1 << 3,   // the selection was made (on the device after RunDevice*)
		kHits = 1 << 4,        // m_hitCount / m_hits / m_hitMasks are this selection's
		kHitText = 1 << 5,     // m_hitText / m_hitTextOffsets are, with the tail m_textTail
		kRoute = 1 << 6,       // the hit lists per regexp were made (on the device after RunDevice*)
		kRouteRows = 1 << 7,   // m_routeCounts / m_routeHits / m_routeSpans are theirs
		kEverything = (1 << 8) - 1
	};
	bool Has(unsigned results) const { return (m_current & results) == results; }
	void Stale(unsigned results) { m_current &= ~results; }
	bool Lines() const { return m_form == kLines || m_form == kLinesField; }
	bool OnDevice() const { return m_form == kDeviceOffsets || m_form == kDeviceStrided; }
	bool SelectionCurrent() const { return Has(kScan | kSelection); }
	bool RouteCurrent() const { return Has(kScan | kRoute); }

	BatchRunner& SetBatch(Form form, const void* text, const uint64_t* offsets, size_t n, size_t len = 0, size_t stride = 0)
	{
		m_form = form;
		m_text = static_cast<const char*>(text);
		m_offsets = offsets;
		m_n = n;
		m_len = len;
		m_stride = stride;
		// (a selection outlives a new batch of strings, as it always has here: SelectionCurrent() looks at the scan first, so Hits()
		// right after Run*() select anew, and Hits() after its States() are those of the batch before -- tests/cpp/shim_calls_test.cpp)
		Stale(Lines() ? kEverything : kEverything & ~(kSelection | kHits | kHitText));
		m_context.NewBatch();
		m_files.NewBatch();
		return *this;
	}

	void Reset()
	{
		m_form = kHostOffsets;
		m_current = 0;
		m_routePitch = 0;
		m_haveWant = false;
		m_hitCount = m_lineCount = 0;
		m_delim = m_sep = 0;
		m_field = m_fieldMode = 0;
		m_textTail = '\n';
		m_flags = 0;
		m_text = nullptr;
		m_offsets = nullptr;
		m_n = m_len = m_stride = 0;
		m_stream = nullptr;
	}

	const uint64_t* Want() const { return m_haveWant ? m_want.data() : nullptr; }
	void SelectFinalsByDefault()
	{
		if (m_want.empty())
			Select();
	}

	void Execute()
	{
		if (Lines())
			throw Pire::Error("pire_hip: RunLines() has hits, no states");
		if (Has(kScan))
			return;
		if (!m_init.empty() && m_init.size() != m_n)
			throw Pire::Error("pire_hip: From() and Run() disagree on the number of strings");
		m_counts.assign(m_table->Regexps() + 2, 0);
		Stale(kStates | kCounts);
		if (OnDevice()) {
			uint32_t* idx = static_cast<uint32_t*>(m_devIdx.Reserve(m_n * 4));
			uint8_t* fin = static_cast<uint8_t*>(m_devFin.Reserve(m_n));
			uint64_t* cnt = static_cast<uint64_t*>(m_devCounts.Reserve(m_counts.size() * 8));
			Check(pire_hip_memset_device(cnt, 0, m_counts.size() * 8, m_stream));
			const uint32_t* init = nullptr;
			if (!m_init.empty()) {
				init = static_cast<const uint32_t*>(m_devInit.Reserve(m_n * 4));
				Check(pire_hip_copy_to_device(m_devInit.Get(), m_init.data(), m_n * 4, m_stream));
			}
			const uint32_t flags = m_flags | PIRE_HIP_RUN_ON_DEVICE;
			if (m_offsets || !m_n)   // (RunDevice() with no offsets is scanned as n records of no bytes, as it always was)
				Check(pire_hip_run(m_table->Handle(), m_text, m_offsets, m_n, flags, init, idx, fin, cnt, m_stream));
			else
				Check(pire_hip_run_strided(m_table->Handle(), m_text, m_n, m_len, m_stride, flags, init, idx, fin, cnt,
				                           m_stream));
			if (!m_init.empty())
				Check(pire_hip_stream_synchronize(m_stream));   // m_init was the source of an asynchronous copy
		} else {
			m_idx.resize(m_n);
			m_fin.resize(m_n);
			Check(pire_hip_run(m_table->Handle(), m_text, OwnedStrings::OffsetsOr(m_offsets, m_n), m_n, m_flags,
			                   m_init.empty() ? nullptr : m_init.data(), m_idx.data(), m_fin.data(), m_counts.data(), nullptr));
			m_current |= kCounts;
		}
		m_current |= kScan;
	}

	/* RunLines(): one call; room for a hit on every line of 64 bytes or more, and a second call where there are more */
	void ExecuteLines()
	{
		if (SelectionCurrent())
			return;
		SelectFinalsByDefault();
		const size_t w = m_want.size();
		GrowAndRetry(m_len / 64 + 1024, [&](size_t cap) {
			m_hits.resize(cap);
			m_hitSpans.resize(cap * 2);
			m_hitMasks.resize(cap * w);
			Check(m_form == kLinesField
			          ? pire_hip_run_lines_field_select(m_table->Handle(), m_text, m_len, m_delim, m_sep, m_field, m_fieldMode, m_flags, Want(),
			                                            &m_lineCount, m_hits.data(), m_hitSpans.data(), m_hitMasks.data(), cap, &m_hitCount,
			                                            nullptr)
			          : pire_hip_run_lines_select(m_table->Handle(), m_text, m_len, m_delim, m_flags, Want(), &m_lineCount, m_hits.data(),
			                                      m_hitSpans.data(), m_hitMasks.data(), cap, &m_hitCount, nullptr));
			return size_t(m_hitCount);
		});
		m_hits.resize(m_hitCount);
		m_hitSpans.resize(m_hitCount * 2);
		m_hitMasks.resize(m_hitCount * w);
		m_current |= kScan | kSelection | kHits;
	}

	/* RunLines(): the selected lines as bytes; room for every byte they can have, and for the hits that are known, or else
	 * ExecuteLines()'s */
	void FetchHitText(char tail)
	{
		if (!Lines())
			throw Pire::Error("pire_hip: HitText() follows RunLines()");
		if (Has(kHitText) && m_textTail == tail)
			return;
		SelectFinalsByDefault();
		uint64_t count = 0, bytes = 0;
		GrowAndRetry(SelectionCurrent() ? size_t(m_hitCount) : m_len / 64 + 1024, [&](size_t cap) {
			m_hitTextOffsets.resize(cap + 1);
			m_hitText.resize(m_len + cap + 1);
			Check(m_form == kLinesField
			          ? pire_hip_run_lines_field_gather(m_table->Handle(), m_text, m_len, m_delim, m_sep, m_field, m_fieldMode, m_flags, Want(),
			                                            uint8_t(tail), &m_lineCount, nullptr, cap, &count, &m_hitText[0], m_hitText.size(),
			                                            m_hitTextOffsets.data(), &bytes, nullptr)
			          : pire_hip_run_lines_gather(m_table->Handle(), m_text, m_len, m_delim, m_flags, Want(), uint8_t(tail), &m_lineCount,
			                                      nullptr, cap, &count, &m_hitText[0], m_hitText.size(), m_hitTextOffsets.data(), &bytes,
			                                      nullptr));
			return size_t(count);   // (the text has room for the whole buffer and a tail per hit: where the hits fit, the bytes do)
		});
		m_hitText.resize(bytes);
		m_hitTextOffsets.resize(count + 1);
		m_textTail = tail;
		m_current |= kHitText;
	}

	/* Context(): the C call of a LineContext::Call, on this runner's table, buffer, flags and selection */
	void ContextCall(const LineContext::Call& c)
	{
		Check(c.gather ? pire_hip_run_lines_context_gather(m_table->Handle(), m_text, m_len, m_delim, m_flags, Want(), c.before, c.after,
		                                                   c.lineCount, c.lines, c.flags, c.spans, c.cap, c.selCount, c.groupCount, c.hitCount,
		                                                   c.tail, c.text, c.textCap, c.offsets, c.bytes, nullptr)
		               : pire_hip_run_lines_context_select(m_table->Handle(), m_text, m_len, m_delim, m_flags, Want(), c.before, c.after,
		                                                   c.lineCount, c.lines, c.flags, c.spans, c.cap, c.selCount, c.groupCount, c.hitCount,
		                                                   nullptr));
	}
	void FetchContext(const char* what)
	{
		SelectFinalsByDefault();
		m_context.FetchLists(what, m_len, [&](const LineContext::Call& c) { ContextCall(c); });
	}
	void FetchContextText(const char* what, char tail)
	{
		SelectFinalsByDefault();
		m_context.FetchText(what, m_len, tail, [&](const LineContext::Call& c) { ContextCall(c); });
	}

	/* Files(): the C call of a LineFiles::Call, on this runner's table, buffer, flags and selection */
	void FilesCall(const LineFiles::Call& c)
	{
		Check(pire_hip_run_lines_files_select(m_table->Handle(), m_text, m_len, m_delim, m_flags, Want(), c.fileBytes, c.files, c.fileMode,
		                                      c.lineCount, c.hits, c.spans, c.hitFile, c.hitLine, c.cap, c.hitCount, c.fileLines, c.fileFirst,
		                                      c.outFiles, c.fileCap, c.fileCount, c.straddles, nullptr));
	}
	void FetchFiles(const char* what)
	{
		SelectFinalsByDefault();
		m_files.FetchLists(what, m_len, [&](const LineFiles::Call& c) { FilesCall(c); });
	}
	void FetchFilesWithout(const char* what)
	{
		SelectFinalsByDefault();
		m_files.FetchWithout(what, [&](const LineFiles::Call& c) { FilesCall(c); });
	}

	void ExecuteSelect()
	{
		if (Lines()) {
			ExecuteLines();
			return;
		}
		const bool current = SelectionCurrent();      // of the scan as it is: Execute() below makes every scan current
		Execute();
		if (current)
			return;
		SelectFinalsByDefault();
		const size_t w = m_want.size();
		if (OnDevice()) {
			uint64_t* hits = static_cast<uint64_t*>(m_devHits.Reserve((m_n + 1) * 8));
			uint64_t* masks = static_cast<uint64_t*>(m_devHitMasks.Reserve((m_n + 1) * w * 8));
			uint64_t* count = static_cast<uint64_t*>(m_devHitCount.Reserve(8));
			const uint64_t* want = nullptr;
			if (m_haveWant) {
				want = static_cast<const uint64_t*>(m_devWant.Reserve(w * 8));
				Check(pire_hip_copy_to_device(m_devWant.Get(), m_want.data(), w * 8, m_stream));
			}
			Check(pire_hip_select(m_table->Handle(), static_cast<const uint32_t*>(m_devIdx.Get()), m_n, want,
			                      PIRE_HIP_RUN_ON_DEVICE, nullptr, hits, masks, m_n, count, m_stream));
			if (m_haveWant)
				Check(pire_hip_stream_synchronize(m_stream));   // m_want was the source of an asynchronous copy
			Stale(kHits);
		} else {
			m_hits.resize(m_n);
			m_hitMasks.resize(m_n * w);
			Check(pire_hip_select(m_table->Handle(), m_idx.data(), m_n, Want(), 0, nullptr, m_hits.data(), m_hitMasks.data(), m_n,
			                      &m_hitCount, nullptr));
			m_hits.resize(m_hitCount);
			m_hitMasks.resize(m_hitCount * w);
			m_current |= kHits;
		}
		m_current |= kSelection;
	}

	void FetchHits()
	{
		ExecuteSelect();
		if (Has(kHits))
			return;
		const size_t w = m_want.size();
		Check(pire_hip_copy_to_host(&m_hitCount, m_devHitCount.Get(), 8, m_stream));
		Check(pire_hip_stream_synchronize(m_stream));
		m_hits.resize(m_hitCount);
		m_hitMasks.resize(m_hitCount * w);
		if (m_hitCount) {
			Check(pire_hip_copy_to_host(m_hits.data(), m_devHits.Get(), m_hitCount * 8, m_stream));
			Check(pire_hip_copy_to_host(m_hitMasks.data(), m_devHitMasks.Get(), m_hitCount * w * 8, m_stream));
			Check(pire_hip_stream_synchronize(m_stream));
		}
		m_current |= kHits;
	}

	/* Rows of a pitch of `pitch` entries (x `width` words) cut to their counts */
	static void CutRows(const std::vector<uint64_t>& flat, const std::vector<uint64_t>& counts, size_t pitch, size_t width,
	                    std::vector<std::vector<uint64_t> >& rows)
	{
		rows.assign(counts.size(), std::vector<uint64_t>());
		for (size_t r = 0; r < counts.size(); ++r)
			rows[r].assign(flat.begin() + r * pitch * width, flat.begin() + (r * pitch + size_t(counts[r])) * width);
	}

	void ExecuteRoute()
	{
		if (RouteCurrent())
			return;
		const size_t regexps = m_table->Regexps();
		m_routeCounts.assign(regexps, 0);
		if (m_form == kLinesField)
			throw Pire::Error("pire_hip: Route() follows Run*() or RunLines(), not RunLinesField()");
		if (Lines()) {
			/* one call; the grow-and-retry of ExecuteLines() on the longest row */
			std::vector<uint64_t> hits, spans;
			m_routePitch = GrowAndRetry(m_len / 64 + 1024, [&](size_t cap) {
				hits.resize(regexps * cap);
				spans.resize(regexps * cap * 2);
				Check(pire_hip_run_lines_route(m_table->Handle(), m_text, m_len, m_delim, m_flags, &m_lineCount, hits.data(), spans.data(),
				                               cap, m_routeCounts.data(), nullptr));
				return regexps ? size_t(*std::max_element(m_routeCounts.begin(), m_routeCounts.end())) : size_t(0);
			});
			CutRows(hits, m_routeCounts, m_routePitch, 1, m_routeHits);
			CutRows(spans, m_routeCounts, m_routePitch, 2, m_routeSpans);
			m_current |= kScan | kRoute | kRouteRows;
			return;
		}
		Execute();
		m_routePitch = m_n;
		if (OnDevice()) {
			uint64_t* hits = static_cast<uint64_t*>(m_devRouteHits.Reserve((regexps * m_n + 1) * 8));
			uint64_t* counts = static_cast<uint64_t*>(m_devRouteCounts.Reserve((regexps + 1) * 8));
			Check(pire_hip_route(m_table->Handle(), static_cast<const uint32_t*>(m_devIdx.Get()), m_n, PIRE_HIP_RUN_ON_DEVICE,
			                     m_n ? hits : nullptr, m_n, counts, m_stream));
			Stale(kRouteRows);
		} else {
			std::vector<uint64_t> hits(regexps * m_n);
			Check(pire_hip_route(m_table->Handle(), m_idx.data(), m_n, 0, m_n ? hits.data() : nullptr, m_n, m_routeCounts.data(), nullptr));
			CutRows(hits, m_routeCounts, m_routePitch, 1, m_routeHits);
			m_current |= kRouteRows;
		}
		m_current |= kRoute;
	}

	void FetchRoute()
	{
		ExecuteRoute();
		if (Has(kRouteRows))
			return;
		const size_t regexps = m_routeCounts.size();
		if (regexps) {
			Check(pire_hip_copy_to_host(m_routeCounts.data(), m_devRouteCounts.Get(), regexps * 8, m_stream));
			Check(pire_hip_stream_synchronize(m_stream));
		}
		m_routeHits.assign(regexps, std::vector<uint64_t>());
		for (size_t r = 0; r < regexps; ++r) {
			m_routeHits[r].resize(size_t(m_routeCounts[r]));
			if (m_routeCounts[r])
				Check(pire_hip_copy_to_host(m_routeHits[r].data(), static_cast<const uint64_t*>(m_devRouteHits.Get()) + r * m_routePitch,
				                            size_t(m_routeCounts[r]) * 8, m_stream));
		}
		Check(pire_hip_stream_synchronize(m_stream));
		m_current |= kRouteRows;
	}

	/* Per-string results on the host, as Scanner::State values. */
	void Fetch()
	{
		Execute();
		if (Has(kStates))
			return;
		if (OnDevice()) {
			m_idx.resize(m_n);
			m_fin.resize(m_n);
			Check(pire_hip_copy_to_host(m_idx.data(), m_devIdx.Get(), m_n * 4, m_stream));
			Check(pire_hip_copy_to_host(m_fin.data(), m_devFin.Get(), m_n, m_stream));
			Check(pire_hip_stream_synchronize(m_stream));
		}
		m_table->ToStates(m_idx, m_states);
		m_final.assign(m_fin.begin(), m_fin.end());
		m_current |= kStates;
	}

	BatchRunner(const BatchRunner&);
	BatchRunner& operator=(const BatchRunner&);

	Table<Scanner>* m_own;
	const Table<Scanner>* m_table;
	uint32_t m_flags;
	Form m_form;                  // the batch: which Run*() set it, and its pointers and sizes
	const char* m_text;
	const uint64_t* m_offsets;
	size_t m_n, m_len, m_stride;
	void* m_stream;
	unsigned m_current;           // Result bits: what is known of the batch
	std::vector<uint32_t> m_init, m_idx;
	std::vector<uint8_t> m_fin;
	std::vector<State> m_states;
	std::vector<char> m_final;
	std::vector<uint64_t> m_counts;
	DeviceBuffer m_devIdx, m_devFin, m_devCounts, m_devInit;
	bool m_haveWant;              // Select() named regexps: m_want goes to the library
	uint8_t m_delim, m_sep;
	uint32_t m_field, m_fieldMode;
	char m_textTail;
	std::string m_hitText;
	std::vector<uint64_t> m_hitTextOffsets;
	uint64_t m_hitCount, m_lineCount;
	std::vector<uint64_t> m_want, m_hits, m_hitMasks, m_hitSpans;
	DeviceBuffer m_devHits, m_devHitMasks, m_devHitCount, m_devWant;
	size_t m_routePitch;
	std::vector<uint64_t> m_routeCounts;
	std::vector<std::vector<uint64_t> > m_routeHits, m_routeSpans;
	DeviceBuffer m_devRouteHits, m_devRouteCounts;
	OwnedStrings m_ownStrings;
	LineContext m_context;        // Context(): the request and what was fetched for it
	LineFiles m_files;            // Files(): the request and what was fetched for it
};

template <class Scanner>
BatchRunner<Scanner>* NewBatchRunner(const Scanner& sc) { return new BatchRunner<Scanner>(sc); }

/*
 * Batched Pire::LongestPrefix / Pire::ShortestPrefix (run.h:277-311).  Returns, per string, the END pointer of the
 * prefix exactly as the reference does (null = no prefix), computed from the lengths the GPU returns.
 */
template <class Scanner>
std::vector<const char*> BatchPrefix(const Table<Scanner>& table, bool longest, const char* text, const uint64_t* offsets,
                                     size_t n, bool throughBeginMark = false, bool throughEndMark = false)
{
	std::vector<int64_t> len(n);
	Check(pire_hip_prefix(table.Handle(), text, OwnedStrings::OffsetsOr(offsets, n), n, longest ? 1 : 0, throughBeginMark ? 1 : 0,
	                      throughEndMark ? 1 : 0, 0, len.data(), nullptr));
	std::vector<const char*> out(n);
	for (size_t i = 0; i < n; ++i)
		out[i] = len[i] < 0 ? nullptr : text + offsets[i] + len[i];
	return out;
}

template <class Scanner>
std::vector<const char*> BatchLongestPrefix(const Table<Scanner>& t, const char* text, const uint64_t* offsets, size_t n,
                                            bool throughBeginMark = false, bool throughEndMark = false)
{
	return BatchPrefix(t, true, text, offsets, n, throughBeginMark, throughEndMark);
}

template <class Scanner>
std::vector<const char*> BatchShortestPrefix(const Table<Scanner>& t, const char* text, const uint64_t* offsets, size_t n,
                                             bool throughBeginMark = false, bool throughEndMark = false)
{
	return BatchPrefix(t, false, text, offsets, n, throughBeginMark, throughEndMark);
}

/*
 * Batched Pire::LongestSuffix / Pire::ShortestSuffix (run.h:313-362): every string is walked backwards from its last
 * byte.  Returns, per string, the pointer the reference returns -- one before the suffix's first byte, i.e.
 * (last byte) - length -- or null.
 */
template <class Scanner>
std::vector<const char*> BatchSuffix(const Table<Scanner>& table, bool longest, const char* text, const uint64_t* offsets,
                                     size_t n, bool throughEndMark = false, bool throughBeginMark = false)
{
	std::vector<int64_t> len(n);
	Check(pire_hip_suffix(table.Handle(), text, OwnedStrings::OffsetsOr(offsets, n), n, longest ? 1 : 0, throughEndMark ? 1 : 0,
	                      throughBeginMark ? 1 : 0, 0, len.data(), nullptr));
	std::vector<const char*> out(n);
	for (size_t i = 0; i < n; ++i)
		out[i] = len[i] < 0 ? nullptr : text + offsets[i + 1] - 1 - len[i];
	return out;
}

template <class Scanner>
std::vector<const char*> BatchLongestSuffix(const Table<Scanner>& t, const char* text, const uint64_t* offsets, size_t n,
                                            bool throughEndMark = false, bool throughBeginMark = false)
{
	return BatchSuffix(t, true, text, offsets, n, throughEndMark, throughBeginMark);
}

template <class Scanner>
std::vector<const char*> BatchShortestSuffix(const Table<Scanner>& t, const char* text, const uint64_t* offsets, size_t n,
                                             bool throughEndMark = false, bool throughBeginMark = false)
{
	return BatchSuffix(t, false, text, offsets, n, throughEndMark, throughBeginMark);
}

/*
 * BatchRunner over every GPU of the node: the batch is cut into one run of whole strings per device,
 * balanced by bytes, staged through buffers the runner keeps between calls, scanned on all devices at once; the match
 * counters are summed with one all-reduce over RCCL (or on the host, Backend() says which).  Same fluent surface:
 *     MultiBatchRunner<Pire::Scanner> gpus(sc);          // all devices; or (sc, {0, 1, 2, 3})
 *     gpus.Begin().Run(lines).End().States()
 */
template <class Scanner>
class MultiBatchRunner {
public:
	typedef typename Scanner::State State;

	explicit MultiBatchRunner(const Scanner& sc, const std::vector<int>& devices = std::vector<int>())
	    : m_table(sc), m_multi(nullptr), m_flags(0), m_text(nullptr), m_offsets(nullptr), m_n(0), m_ran(false)
	{
		Check(pire_hip_multi_create(devices.empty() ? nullptr : devices.data(), int(devices.size()), &m_multi));
	}
	~MultiBatchRunner() { pire_hip_multi_destroy(m_multi); }

	MultiBatchRunner& Begin() { m_flags |= PIRE_HIP_RUN_BEGIN; return *this; }
	MultiBatchRunner& End() { m_flags |= PIRE_HIP_RUN_END; return *this; }
	MultiBatchRunner& Run(const char* text, const uint64_t* offsets, size_t n)
	{
		m_text = text;
		m_offsets = offsets;
		m_n = n;
		m_ran = false;
		return *this;
	}
	MultiBatchRunner& Run(const std::vector<ystring>& strings)
	{
		m_ownStrings.Assign(strings);
		return Run(m_ownStrings.Text(), m_ownStrings.Offsets(), strings.size());
	}
	const std::vector<State>& States() { Execute(); return m_states; }
	const std::vector<char>& Finals() { Execute(); return m_final; }
	const std::vector<uint64_t>& MatchCounts() { Execute(); return m_counts; }
	int Devices() const { return pire_hip_multi_device_count(m_multi); }
	const char* Backend() const { return pire_hip_multi_reduce_backend(m_multi); }
	Table<Scanner>& GetTable() { return m_table; }

private:
	MultiBatchRunner(const MultiBatchRunner&);
	MultiBatchRunner& operator=(const MultiBatchRunner&);
	void Execute()
	{
		if (m_ran)
			return;
		std::vector<uint32_t> idx(m_n);
		std::vector<uint8_t> fin(m_n);
		m_counts.assign(m_table.Regexps() + 2, 0);
		Check(pire_hip_multi_run_host(m_multi, m_table.Handle(), m_text, OwnedStrings::OffsetsOr(m_offsets, m_n), m_n, m_flags, nullptr,
		                              idx.data(), fin.data(), m_counts.data()));
		m_table.ToStates(idx, m_states);
		m_final.assign(fin.begin(), fin.end());
		m_ran = true;
	}

	Table<Scanner> m_table;
	pire_hip_multi* m_multi;
	uint32_t m_flags;
	const char* m_text;
	const uint64_t* m_offsets;
	size_t m_n;
	bool m_ran;
	OwnedStrings m_ownStrings;
	std::vector<State> m_states;
	std::vector<char> m_final;
	std::vector<uint64_t> m_counts;
};

/*
 * Batched twin of Pire::ScannerPair<Scanner1, Scanner2> (scanners/pair.h:33-94) and of
 * Pire::Run(scanner1, scanner2, state1, state2, begin, end) (run.h:229-241): both scanners over the same strings, State =
 * pair of the two states (pair.h:35), Final = either (pair.h:69-72).  Host pointers: two passes (the walks are
 * independent, pair.h:52-66).  Device-resident fixed-length records (RunDeviceStrided): ONE fused pass with both tables
 * in LDS -- the text is read once (pire_hip_run_pair_strided).
 */
template <class Scanner1, class Scanner2>
class PairBatchRunner {
public:
	typedef ypair<typename Scanner1::State, typename Scanner2::State> State;

	PairBatchRunner(const Scanner1& s1, const Scanner2& s2)
	    : m_first(s1), m_second(s2), m_fused(false), m_ran(false), m_text(nullptr), m_n(0), m_len(0), m_stride(0), m_stream(nullptr) {}

	PairBatchRunner& Begin() { m_first.Begin(); m_second.Begin(); return *this; }
	PairBatchRunner& End() { m_first.End(); m_second.End(); return *this; }
	PairBatchRunner& Run(const char* text, const uint64_t* offsets, size_t n)
	{
		m_fused = false;
		m_first.Run(text, offsets, n);
		m_second.Run(text, offsets, n);
		return *this;
	}
	PairBatchRunner& Run(const std::vector<ystring>& strings)
	{
		m_fused = false;
		m_first.Run(strings);
		m_second.Run(strings);
		return *this;
	}
	/* Device-resident fixed-length records: one fused pass. */
	PairBatchRunner& RunDeviceStrided(const void* deviceText, size_t n, size_t len, size_t stride, void* stream = nullptr)
	{
		m_fused = true;
		m_ran = false;
		m_text = deviceText;
		m_n = n;
		m_len = len;
		m_stride = stride;
		m_stream = stream;
		return *this;
	}

	/* RunHelper<ScannerPair>::State() per string. */
	std::vector<State> States()
	{
		if (m_fused)
			ExecuteFused();
		const std::vector<typename Scanner1::State>& a = m_fused ? m_states1 : m_first.States();
		const std::vector<typename Scanner2::State>& b = m_fused ? m_states2 : m_second.States();
		std::vector<State> out(a.size());
		for (size_t i = 0; i < a.size(); ++i)
			out[i] = ymake_pair(a[i], b[i]);
		return out;
	}
	/* ScannerPair::Final per string (pair.h:69-72). */
	std::vector<char> Finals()
	{
		if (m_fused) {
			ExecuteFused();
			return std::vector<char>(m_fin.begin(), m_fin.end());
		}
		const std::vector<char>& a = m_first.Finals();
		const std::vector<char>& b = m_second.Finals();
		std::vector<char> out(a.size());
		for (size_t i = 0; i < a.size(); ++i)
			out[i] = char(a[i] || b[i]);
		return out;
	}
	BatchRunner<Scanner1>& First() { return m_first; }
	BatchRunner<Scanner2>& Second() { return m_second; }

private:
	void ExecuteFused()
	{
		if (m_ran)
			return;
		uint32_t* d1 = static_cast<uint32_t*>(m_dev1.Reserve(m_n * 4));
		uint32_t* d2 = static_cast<uint32_t*>(m_dev2.Reserve(m_n * 4));
		uint8_t* df = static_cast<uint8_t*>(m_devFin.Reserve(m_n));
		Check(pire_hip_run_pair_strided(m_first.GetTable().Handle(), m_second.GetTable().Handle(), m_text, m_n, m_len, m_stride,
		                                m_first.Flags() | PIRE_HIP_RUN_ON_DEVICE, d1, d2, df, m_stream));
		std::vector<uint32_t> idx1(m_n), idx2(m_n);
		m_fin.resize(m_n);
		Check(pire_hip_copy_to_host(idx1.data(), d1, m_n * 4, m_stream));
		Check(pire_hip_copy_to_host(idx2.data(), d2, m_n * 4, m_stream));
		Check(pire_hip_copy_to_host(m_fin.data(), df, m_n, m_stream));
		Check(pire_hip_stream_synchronize(m_stream));
		m_first.GetTable().ToStates(idx1, m_states1);
		m_second.GetTable().ToStates(idx2, m_states2);
		m_ran = true;
	}

	BatchRunner<Scanner1> m_first;
	BatchRunner<Scanner2> m_second;
	bool m_fused, m_ran;
	const void* m_text;
	size_t m_n, m_len, m_stride;
	void* m_stream;
	std::vector<typename Scanner1::State> m_states1;
	std::vector<typename Scanner2::State> m_states2;
	std::vector<uint8_t> m_fin;
	DeviceBuffer m_dev1, m_dev2, m_devFin;
};

/*
 * What HalfFinalBatchRunner and CountingBatchRunner below are: a batched Runner whose scanner counts -- per string the
 * per-regexp counts State::Result(r), plus StateIndex of the end state.  A scanner's State is an opaque class with private
 * members, so the results come back as plain numbers.  Derived keeps its table and its three C calls, as
 *     int Scan(offsets, out_idx, out_results)                                 the scan of m_n strings of m_text
 *     int SelectStrings(offsets, min, mode, totals, hits, rows, cap, count)   the same, selected on the device
 *     int SelectLines(min, mode, lineCount, totals, hits, spans, rows, cap, count)    of the m_len bytes of m_text, cut at m_delim
 * and is what the fluent calls return.
 */
template <class Derived>
class CountedBatchRunner {
public:
	Derived& Begin() { m_flags |= PIRE_HIP_RUN_BEGIN; return Self(); }
	Derived& End() { m_flags |= PIRE_HIP_RUN_END; return Self(); }
	Derived& Run(const char* text, const uint64_t* offsets, size_t n)
	{
		m_text = text;
		m_offsets = offsets;
		m_n = n;
		m_lines = false;
		m_ran = m_selected = false;
		return Self();
	}
	Derived& Run(const std::vector<ystring>& strings)
	{
		m_ownStrings.Assign(strings);
		return Run(m_ownStrings.Text(), m_ownStrings.Offsets(), strings.size());
	}

	/* State::Result(r) of string i. */
	size_t Result(size_t i, size_t r) { Execute(); return m_results[i * m_regexps + r]; }
	const std::vector<uint32_t>& Results() { Execute(); return m_results; }       // [n][RegexpsCount()]
	const std::vector<uint32_t>& StateIndices() { Execute(); return m_idx; }      // StateIndex(State()) per string

	/*
	 * The strings whose counts reach their thresholds, without a loop on the host (pire_hip_count_select behind the scan;
	 * include/pire_hip.h, "the strings that count, on the device"):
	 *     run.Begin().Run(text, offsets, n).End().Select();    // the strings in which some regexp occurred
	 *     run.Select({3, 0, 1});                                // ... regexp 0 three times or regexp 2 once (0 = not asked)
	 *     run.Select({3, 0, 1}, true);                          // ... and regexp 2 once
	 *     run.Hits()        the selected strings, ascending      run.HitResults()  their result rows, [k][RegexpsCount()]
	 *     run.HitCount()    how many                             run.Totals()      occurrences per regexp over ALL strings
	 *     run.Begin().RunLines(raw, size).End();                // the same per line of raw, split on the device, and
	 *     run.HitSpans()    [2 * k], [2 * k + 1]: line Hits()[k] is raw[begin, end)        run.LineCount()  lines in the buffer
	 * After RunLines() there are hits only: Result() / Results() / StateIndices() throw.
	 */
	Derived& Select(const std::vector<uint32_t>& min = std::vector<uint32_t>(), bool all = false)
	{
		m_min = min;
		m_all = all;
		m_selected = false;
		return Self();
	}
	Derived& RunLines(const char* raw, size_t size, char delim = '\n')
	{
		m_text = raw;
		m_len = size;
		m_delim = uint8_t(delim);
		m_lines = true;
		m_ran = m_selected = false;
		return Self();
	}
	const std::vector<uint64_t>& Hits() { FetchHits(); return m_hits; }
	const std::vector<uint32_t>& HitResults() { FetchHits(); return m_rows; }
	size_t HitCount() { FetchHits(); return size_t(m_hitCount); }
	const std::vector<uint64_t>& Totals() { FetchHits(); return m_totals; }
	const std::vector<uint64_t>& HitSpans()
	{
		if (!m_lines)
			throw Pire::Error("pire_hip: HitSpans() follows RunLines()");
		FetchHits();
		return m_spans;
	}
	size_t LineCount()
	{
		if (!m_lines)
			throw Pire::Error("pire_hip: LineCount() follows RunLines()");
		FetchHits();
		return size_t(m_lineCount);
	}

protected:
	explicit CountedBatchRunner(size_t regexps)
	    : m_regexps(regexps), m_flags(0), m_text(nullptr), m_offsets(nullptr), m_n(0), m_len(0), m_delim('\n'), m_lines(false), m_ran(false),
	      m_selected(false), m_all(false), m_hitCount(0), m_lineCount(0) {}

	void Execute()
	{
		if (m_ran)
			return;
		if (m_lines)
			throw Pire::Error("pire_hip: RunLines() has hits, no results per string");
		m_idx.assign(m_n, 0);
		m_results.assign(m_n * (m_regexps ? m_regexps : 1), 0);
		Check(Self().Scan(OwnedStrings::OffsetsOr(m_offsets, m_n), m_idx.data(), m_results.data()));
		m_ran = true;
	}

	size_t m_regexps;
	uint32_t m_flags;
	const char* m_text;           // Run(): the strings' text; RunLines(): the raw buffer of m_len bytes
	const uint64_t* m_offsets;
	size_t m_n, m_len;
	uint8_t m_delim;

private:
	Derived& Self() { return static_cast<Derived&>(*this); }

	/* One call with room for every string -- RunLines(): for a hit on every line of 64 bytes or more --, and a second one where
	 * there are more */
	void FetchHits()
	{
		if (m_selected)
			return;
		if (!m_min.empty() && m_min.size() != m_regexps)
			throw Pire::Error("pire_hip: Select() takes one threshold per regexp");
		m_totals.assign(m_regexps, 0);
		GrowAndRetry(m_lines ? m_len / 64 + 16 : m_n, [&](size_t room) {
			m_hits.assign(room, 0);
			m_rows.assign(room * m_regexps, 0);
			m_spans.assign(m_lines ? 2 * room : 0, 0);
			const uint32_t* min = m_min.empty() ? nullptr : m_min.data();
			const uint32_t mode = m_all ? PIRE_HIP_COUNT_ALL : 0u;
			uint64_t* totals = m_regexps ? m_totals.data() : nullptr;
			uint64_t* hits = room ? m_hits.data() : nullptr;
			uint32_t* rows = room && m_regexps ? m_rows.data() : nullptr;
			Check(m_lines ? Self().SelectLines(min, mode, &m_lineCount, totals, hits, room ? m_spans.data() : nullptr, rows, room, &m_hitCount)
			              : Self().SelectStrings(OwnedStrings::OffsetsOr(m_offsets, m_n), min, mode, totals, hits, rows, room, &m_hitCount));
			return size_t(m_hitCount);
		});
		m_hits.resize(size_t(m_hitCount));
		m_rows.resize(size_t(m_hitCount) * m_regexps);
		m_spans.resize(m_lines ? 2 * size_t(m_hitCount) : 0);
		m_selected = true;
	}

	bool m_lines, m_ran, m_selected;
	bool m_all;                   // Select(): the thresholds, and whether all of them have to be reached
	std::vector<uint32_t> m_min;
	std::vector<uint32_t> m_idx, m_results, m_rows;
	std::vector<uint64_t> m_hits, m_spans, m_totals;
	uint64_t m_hitCount, m_lineCount;
	OwnedStrings m_ownStrings;
};

/*
 * Batched Runner over a Pire::HalfFinalScanner (scanners/half_final.h): per string the per-regexp match counts
 * State::Result(r) (half_final.h:90-92) that Initialize + Begin() + Run() + End() accumulate through TakeAction
 * (half_final.h:137-164), plus Final and StateIndex of the end state.  The calls are CountedBatchRunner's.
 */
template <class HalfScanner = Pire::HalfFinalScanner>
class HalfFinalBatchRunner : public CountedBatchRunner<HalfFinalBatchRunner<HalfScanner> > {
public:
	explicit HalfFinalBatchRunner(const HalfScanner& sc)
	    : CountedBatchRunner<HalfFinalBatchRunner>(sc.RegexpsCount()), m_table(nullptr)
	{
		const std::string blob = SavedBlob(sc);
		Check(pire_hip_table_create(blob.data(), blob.size(), &m_table));
	}
	~HalfFinalBatchRunner() { pire_hip_table_destroy(m_table); }

	const std::vector<char>& Finals() { this->Execute(); return m_final; }        // Final(State()) per string

private:
	friend class CountedBatchRunner<HalfFinalBatchRunner>;
	int Scan(const uint64_t* offsets, uint32_t* idx, uint32_t* results)
	{
		std::vector<uint8_t> fin(this->m_n);
		const int rc = pire_hip_run_half_final(m_table, this->m_text, offsets, this->m_n, this->m_flags, idx, fin.data(), results, nullptr);
		m_final.assign(fin.begin(), fin.end());
		return rc;
	}
	int SelectStrings(const uint64_t* offsets, const uint32_t* min, uint32_t mode, uint64_t* totals, uint64_t* hits, uint32_t* rows, uint64_t cap,
	                  uint64_t* count)
	{
		return pire_hip_run_half_final_select(m_table, this->m_text, offsets, this->m_n, this->m_flags, nullptr, nullptr, nullptr, min, mode,
		                                      totals, hits, rows, cap, count, nullptr);
	}
	int SelectLines(const uint32_t* min, uint32_t mode, uint64_t* lineCount, uint64_t* totals, uint64_t* hits, uint64_t* spans, uint32_t* rows,
	                uint64_t cap, uint64_t* count)
	{
		return pire_hip_half_final_lines_select(m_table, this->m_text, this->m_len, this->m_delim, this->m_flags, min, mode, lineCount, totals,
		                                        hits, spans, rows, cap, count, nullptr);
	}

	HalfFinalBatchRunner(const HalfFinalBatchRunner&);
	HalfFinalBatchRunner& operator=(const HalfFinalBatchRunner&);
	pire_hip_table* m_table;
	std::vector<char> m_final;
};

/*
 * Batched Runner over a Pire::CountingScanner, AdvancedCountingScanner or NoGlueLimitCountingScanner (extra/count.h; include <pire/extra.h>
 * before this header): per string State::Result(r) for every glued regexp (count.h:206) after
 * Initialize + Begin() + Run() + End(), as tests/count_ut.cpp:54-63 drives them.  The calls are CountedBatchRunner's.
 */
#ifdef PIRE_EXTRA_COUNT_H
template <class CountScanner>
struct CountingKind;
template <>
struct CountingKind<Pire::CountingScanner> {
	enum { Value = PIRE_HIP_COUNTING_BASIC };
};
template <>
struct CountingKind<Pire::AdvancedCountingScanner> {
	enum { Value = PIRE_HIP_COUNTING_ADVANCED };
};
template <>
struct CountingKind<Pire::NoGlueLimitCountingScanner> {
	enum { Value = PIRE_HIP_COUNTING_NOGLUELIMIT };
};

template <class CountScanner>
class CountingBatchRunner : public CountedBatchRunner<CountingBatchRunner<CountScanner> > {
public:
	explicit CountingBatchRunner(const CountScanner& sc)
	    : CountedBatchRunner<CountingBatchRunner>(sc.RegexpsCount()), m_table(nullptr)
	{
		const std::string blob = SavedBlob(sc);
		Check(pire_hip_counting_table_create(blob.data(), blob.size(), &m_table));
	}
	~CountingBatchRunner() { pire_hip_counting_table_destroy(m_table); }

private:
	friend class CountedBatchRunner<CountingBatchRunner>;
	enum { Kind = CountingKind<CountScanner>::Value };
	int Scan(const uint64_t* offsets, uint32_t* idx, uint32_t* results)
	{
		return pire_hip_counting_run(m_table, Kind, this->m_text, offsets, this->m_n, this->m_flags, idx, results, nullptr);
	}
	int SelectStrings(const uint64_t* offsets, const uint32_t* min, uint32_t mode, uint64_t* totals, uint64_t* hits, uint32_t* rows, uint64_t cap,
	                  uint64_t* count)
	{
		return pire_hip_counting_run_select(m_table, Kind, this->m_text, offsets, this->m_n, this->m_flags, nullptr, nullptr, min, mode, totals,
		                                    hits, rows, cap, count, nullptr);
	}
	int SelectLines(const uint32_t* min, uint32_t mode, uint64_t* lineCount, uint64_t* totals, uint64_t* hits, uint64_t* spans, uint32_t* rows,
	                uint64_t cap, uint64_t* count)
	{
		return pire_hip_counting_lines_select(m_table, Kind, this->m_text, this->m_len, this->m_delim, this->m_flags, min, mode, lineCount,
		                                      totals, hits, spans, rows, cap, count, nullptr);
	}

	CountingBatchRunner(const CountingBatchRunner&);
	CountingBatchRunner& operator=(const CountingBatchRunner&);
	pire_hip_counting_table* m_table;
};
#endif  // PIRE_EXTRA_COUNT_H

/*
 * Batched Runner over a Pire::CapturingScanner (extra/capture.h:49-162; include <pire/extra.h> before this header):
 * per string State::Captured(), Begin(), End() and Final after Initialize + Begin() + Run() + End(), as
 * tests/capture_ut.cpp:75-83 drives it.  The captured text of string i is
 * [text + offsets[i] + Begin(i) - 1, text + offsets[i] + End(i) - 1) (capture_ut.cpp:85-91).
 * The captured substrings without a loop on the host (include/pire_hip.h, "the captured substrings, on the device"):
 *     run.Begin().Run(text, offsets, n).End();      run.CapturedLines()  the strings that captured, ascending
 *                                                   run.CapturedSpans()  [begin, end) of their captured text in `text`, 2 per string
 *     run.Begin().RunLines(raw, size).End();        the same per line of raw (spans: byte ranges of raw), and
 *     run.CapturedText()                            the captured fields back to back, '\n' (or the byte given) behind each:
 *                                                   `grep -o` with one pair of parentheses, gathered on the device
 *     run.CapturedTextOffsets()                     field k is CapturedText()[o[k], o[k + 1])
 */
#ifdef PIRE_EXTRA_CAPTURE_H
class CaptureBatchRunner {
public:
	explicit CaptureBatchRunner(const Pire::CapturingScanner& sc)
	    : m_table(nullptr), m_flags(0), m_text(nullptr), m_offsets(nullptr), m_n(0), m_ran(false), m_lines(false), m_len(0),
	      m_delim('\n'), m_listed(false), m_textFetched(false), m_textTail('\n'), m_lineCount(0)
	{
		const std::string blob = SavedBlob(sc);
		Check(pire_hip_counting_table_create(blob.data(), blob.size(), &m_table));
	}
	~CaptureBatchRunner() { pire_hip_counting_table_destroy(m_table); }

	CaptureBatchRunner& Begin() { m_flags |= PIRE_HIP_RUN_BEGIN; return *this; }
	CaptureBatchRunner& End() { m_flags |= PIRE_HIP_RUN_END; return *this; }
	CaptureBatchRunner& Run(const char* text, const uint64_t* offsets, size_t n)
	{
		m_text = text;
		m_offsets = offsets;
		m_n = n;
		m_ran = m_lines = m_listed = m_textFetched = false;
		return *this;
	}
	/* One raw buffer, cut into lines at `delim` on the device; the accessors per string do not follow it */
	CaptureBatchRunner& RunLines(const char* raw, size_t size, char delim = '\n')
	{
		m_text = raw;
		m_len = size;
		m_delim = uint8_t(delim);
		m_lines = true;
		m_ran = m_listed = m_textFetched = false;
		return *this;
	}
	CaptureBatchRunner& Run(const std::vector<ystring>& strings)
	{
		m_ownStrings.Assign(strings);
		return Run(m_ownStrings.Text(), m_ownStrings.Offsets(), strings.size());
	}

	bool Captured(size_t i) { Execute(); return m_begin[i] >= 0 && m_end[i] >= 0; }     // State::Captured()
	size_t Begin(size_t i) { Execute(); return size_t(m_begin[i]); }                    // State::Begin() (npos if unset)
	size_t End(size_t i) { Execute(); return size_t(m_end[i]); }                        // State::End()
	bool Final(size_t i) { Execute(); return m_final[i] != 0; }
	size_t StateIndex(size_t i) { Execute(); return m_idx[i]; }

	const std::vector<uint64_t>& CapturedLines() { FetchList(); return m_hits; }
	const std::vector<uint64_t>& CapturedSpans() { FetchList(); return m_spans; }
	size_t LineCount() { FetchList(); return size_t(m_lineCount); }
	const std::string& CapturedText(char tail = '\n') { FetchText(tail); return m_capturedText; }
	const std::vector<uint64_t>& CapturedTextOffsets()
	{
		if (!m_textFetched)
			FetchText('\n');
		return m_capturedOffsets;
	}

private:
	void ResultsPerString()
	{
		m_idx.assign(m_n, 0);
		m_final.assign(m_n, 0);
		m_begin.assign(m_n, -1);
		m_end.assign(m_n, -1);
	}

	void Execute()
	{
		if (m_lines)
			throw Pire::Error("pire_hip: the accessors per string follow Run(), not RunLines()");
		if (m_ran)
			return;
		ResultsPerString();
		Check(pire_hip_capture_run(m_table, m_text, OwnedStrings::OffsetsOr(m_offsets, m_n), m_n, m_flags, m_idx.data(), m_final.data(),
		                           m_begin.data(), m_end.data(), nullptr));
		m_ran = true;
	}

	/* The list of the strings (lines) that captured and their spans: one call -- for RunLines() with room for a capture on
	 * every line of 64 bytes or more, and a second call where there are more */
	void FetchList()
	{
		if (m_listed)
			return;
		uint64_t count = 0;
		if (!m_lines) {
			ResultsPerString();
			m_hits.resize(m_n);
			m_spans.resize(m_n * 2);
			Check(pire_hip_capture_run_select(m_table, m_text, OwnedStrings::OffsetsOr(m_offsets, m_n), m_n, m_flags, 0, m_idx.data(),
			                                  m_final.data(), m_begin.data(), m_end.data(), m_hits.data(), m_spans.data(), m_n, &count, nullptr));
			m_lineCount = m_n;
			m_ran = true;
		} else {
			GrowAndRetry(m_len / 64 + 1024, [&](size_t cap) {
				m_hits.resize(cap);
				m_spans.resize(cap * 2);
				Check(pire_hip_capture_lines_gather(m_table, m_text, m_len, m_delim, m_flags, 0, PIRE_HIP_GATHER_NO_TAIL, &m_lineCount,
				                                    m_hits.data(), m_spans.data(), cap, &count, nullptr, 0, nullptr, nullptr, nullptr));
				return size_t(count);
			});
		}
		m_hits.resize(count);
		m_spans.resize(count * 2);
		m_listed = true;
	}

	/* RunLines(): the captured fields as bytes (and the list with them); room for the list that is known, or else FetchList()'s */
	void FetchText(char tail)
	{
		if (!m_lines)
			throw Pire::Error("pire_hip: CapturedText() follows RunLines()");
		if (m_textFetched && m_textTail == tail)
			return;
		uint64_t count = 0, bytes = 0;
		GrowAndRetry(m_listed ? m_hits.size() : m_len / 64 + 1024, [&](size_t cap) {
			m_hits.resize(cap);
			m_spans.resize(cap * 2);
			m_capturedOffsets.resize(cap + 1);
			m_capturedText.resize(m_len + cap + 1);
			Check(pire_hip_capture_lines_gather(m_table, m_text, m_len, m_delim, m_flags, 0, uint8_t(tail), &m_lineCount, m_hits.data(),
			                                    m_spans.data(), cap, &count, &m_capturedText[0], m_capturedText.size(),
			                                    m_capturedOffsets.data(), &bytes, nullptr));
			return size_t(count);   // (the bytes fit where the hits do, as in BatchRunner::FetchHitText())
		});
		m_hits.resize(count);
		m_spans.resize(count * 2);
		m_capturedText.resize(bytes);
		m_capturedOffsets.resize(count + 1);
		m_textTail = tail;
		m_listed = m_textFetched = true;
	}

	CaptureBatchRunner(const CaptureBatchRunner&);
	CaptureBatchRunner& operator=(const CaptureBatchRunner&);
	pire_hip_counting_table* m_table;
	uint32_t m_flags;
	const char* m_text;
	const uint64_t* m_offsets;
	size_t m_n;
	bool m_ran;
	std::vector<uint32_t> m_idx;
	std::vector<uint8_t> m_final;
	std::vector<int64_t> m_begin, m_end;
	OwnedStrings m_ownStrings;
	bool m_lines;                 // RunLines(): m_text is the raw buffer of m_len bytes
	size_t m_len;
	uint8_t m_delim;
	bool m_listed, m_textFetched;
	char m_textTail;
	uint64_t m_lineCount;
	std::vector<uint64_t> m_hits, m_spans, m_capturedOffsets;
	std::string m_capturedText;
};

/*
 * Batched runs of a Pire::SlowCapturingScanner (extra/capture.h:170-581): Initialize, Run, GetCapture per string -- the
 * scanner that tells .*?(re) from .*(re).  It takes the begin and end marks itself: there is no Begin() / End() here.
 *     Pire::Hip::SlowCaptureBatchRunner run(sc);            // Save() -> pire_hip_slow_capture_table_create()
 *     run.Run(text, offsets, n);   run.Run(strings);
 *     run.Captured(i)   GetCapture()'s return        run.Matched(i)   whether it assigned `final`
 *     run.Begin(i)  run.End(i)                       final.GetBegin() / GetEnd(): the captured text is string i [begin, end)
 *     run.Select();     run.Hits()      the strings that captured, ascending        run.HitCount()
 *                       run.HitSpans()  [2 * k], [2 * k + 1]: the capture of hit k as a byte range of the text (Run()) or of raw
 *     run.RunLines(raw, size);          one raw buffer cut into lines on the device (pire_hip_slow_capture_lines_gather)
 *     run.LineCount()   run.HitText()   the captured fields back to back, '\n' (or the byte given) behind each: `grep -o` with
 *                       lazy quantifiers                 run.HitTextOffsets()  field k is HitText()[o[k], o[k + 1])
 * The caller's arrays are read when an accessor first asks: they live until then.  What the library refuses comes back as
 * Pire::Error.
 */
class SlowCaptureBatchRunner {
public:
	explicit SlowCaptureBatchRunner(const Pire::SlowCapturingScanner& sc)
	    : m_table(nullptr), m_form(kNone), m_text(nullptr), m_offsets(nullptr), m_n(0), m_len(0), m_delim('\n'), m_ran(false),
	      m_listed(false), m_haveText(false), m_textTail('\n'), m_hitCount(0), m_lineCount(0)
	{
		const std::string blob = SavedBlob(sc);
		Check(pire_hip_slow_capture_table_create(blob.data(), blob.size(), &m_table));
	}
	~SlowCaptureBatchRunner() { pire_hip_slow_capture_table_destroy(m_table); }

	SlowCaptureBatchRunner& Run(const char* text, const uint64_t* offsets, size_t n) { return SetBatch(kStrings, text, offsets, n, 0, '\n'); }
	SlowCaptureBatchRunner& Run(const std::vector<ystring>& strings)
	{
		m_ownStrings.Assign(strings);
		return Run(m_ownStrings.Text(), m_ownStrings.Offsets(), strings.size());
	}
	SlowCaptureBatchRunner& RunLines(const char* raw, size_t size, char delim = '\n') { return SetBatch(kLines, raw, nullptr, 0, size, delim); }
	/* The list of the strings (lines) that captured: fetched with the first accessor that asks */
	SlowCaptureBatchRunner& Select()
	{
		m_listed = m_haveText = false;
		return *this;
	}

	bool Captured(size_t i) { Execute(); return m_captured[i] != 0; }
	bool Matched(size_t i) { Execute(); return m_matched[i] != 0; }
	size_t Begin(size_t i) { Execute(); return size_t(m_begin[i]); }      // (npos if unset)
	size_t End(size_t i) { Execute(); return size_t(m_end[i]); }

	uint64_t HitCount() { FetchHits(); return m_hitCount; }
	const std::vector<uint64_t>& Hits() { FetchHits(); return m_hits; }
	const std::vector<uint64_t>& HitSpans() { FetchHits(); return m_hitSpans; }
	uint64_t LineCount() { NeedLines("LineCount()"); FetchHits(); return m_lineCount; }
	const std::string& HitText(char tail = '\n') { FetchHitText(tail); return m_hitText; }
	const std::vector<uint64_t>& HitTextOffsets()
	{
		if (!m_haveText)
			FetchHitText('\n');
		return m_hitTextOffsets;
	}

private:
	SlowCaptureBatchRunner(const SlowCaptureBatchRunner&);
	SlowCaptureBatchRunner& operator=(const SlowCaptureBatchRunner&);

	enum Form { kNone, kStrings, kLines };
	SlowCaptureBatchRunner& SetBatch(Form form, const char* text, const uint64_t* offsets, size_t n, size_t len, char delim)
	{
		m_form = form, m_text = text, m_offsets = offsets, m_n = n, m_len = len, m_delim = uint8_t(delim);
		m_ran = m_listed = m_haveText = false;
		return *this;
	}
	void NeedLines(const char* what) const
	{
		if (m_form != kLines)
			throw Pire::Error(std::string("pire_hip: ") + what + " follows RunLines()");
	}
	void ResultsPerString()
	{
		m_captured.assign(m_n, 0);
		m_matched.assign(m_n, 0);
		m_begin.assign(m_n, -1);
		m_end.assign(m_n, -1);
	}
	void Execute()
	{
		if (m_form != kStrings)
			throw Pire::Error("pire_hip: the accessors per string follow Run()");
		if (m_ran)
			return;
		ResultsPerString();
		Check(pire_hip_slow_capture_run(m_table, m_text, OwnedStrings::OffsetsOr(m_offsets, m_n), m_n, 0, m_captured.data(), m_begin.data(),
		                                m_end.data(), m_matched.data(), nullptr));
		m_ran = true;
	}
	/* Run(): one call with room for every string, which leaves the answers per string as well.  RunLines(): room for a capture
	 * on every line of 64 bytes or more, and a second call where there are more */
	void FetchHits()
	{
		if (m_listed)
			return;
		if (m_form == kNone)
			throw Pire::Error("pire_hip: Hits() follows Run() or RunLines()");
		if (m_form == kStrings) {
			ResultsPerString();
			m_hits.resize(m_n);
			m_hitSpans.resize(m_n * 2);
			Check(pire_hip_slow_capture_run_select(m_table, m_text, OwnedStrings::OffsetsOr(m_offsets, m_n), m_n, 0, m_captured.data(),
			                                       m_begin.data(), m_end.data(), m_matched.data(), m_hits.data(), m_hitSpans.data(), m_n,
			                                       &m_hitCount, nullptr));
			m_ran = true;
		} else {
			GrowAndRetry(m_len / 64 + 1024, [&](size_t cap) {
				m_hits.resize(cap);
				m_hitSpans.resize(cap * 2);
				Check(pire_hip_slow_capture_lines_gather(m_table, m_text, m_len, m_delim, 0, PIRE_HIP_GATHER_NO_TAIL, &m_lineCount, m_hits.data(),
				                                         m_hitSpans.data(), cap, &m_hitCount, nullptr, 0, nullptr, nullptr, nullptr));
				return size_t(m_hitCount);
			});
		}
		m_hits.resize(m_hitCount);
		m_hitSpans.resize(m_hitCount * 2);
		m_listed = true;
	}
	/* RunLines(): the captured fields as bytes (and the list with them) */
	void FetchHitText(char tail)
	{
		NeedLines("HitText()");
		if (m_haveText && m_textTail == tail)
			return;
		uint64_t bytes = 0;
		GrowAndRetry(m_listed ? size_t(m_hitCount) : m_len / 64 + 1024, [&](size_t cap) {
			m_hits.resize(cap);
			m_hitSpans.resize(cap * 2);
			m_hitTextOffsets.resize(cap + 1);
			m_hitText.resize(m_len + cap + 1);
			Check(pire_hip_slow_capture_lines_gather(m_table, m_text, m_len, m_delim, 0, uint8_t(tail), &m_lineCount, m_hits.data(),
			                                         m_hitSpans.data(), cap, &m_hitCount, &m_hitText[0], m_hitText.size(),
			                                         m_hitTextOffsets.data(), &bytes, nullptr));
			return size_t(m_hitCount);   // (the bytes fit where the hits do, as in BatchRunner::FetchHitText())
		});
		m_hits.resize(m_hitCount);
		m_hitSpans.resize(m_hitCount * 2);
		m_hitText.resize(bytes);
		m_hitTextOffsets.resize(m_hitCount + 1);
		m_textTail = tail;
		m_listed = m_haveText = true;
	}

	pire_hip_slow_capture_table* m_table;
	Form m_form;
	const char* m_text;           // Run(): the strings' text; RunLines(): the raw buffer of m_len bytes
	const uint64_t* m_offsets;
	size_t m_n, m_len;
	uint8_t m_delim;
	bool m_ran, m_listed, m_haveText;
	char m_textTail;
	OwnedStrings m_ownStrings;
	uint64_t m_hitCount, m_lineCount;
	std::vector<uint8_t> m_captured, m_matched;
	std::vector<int64_t> m_begin, m_end;
	std::vector<uint64_t> m_hits, m_hitSpans, m_hitTextOffsets;
	std::string m_hitText;
};
#endif  // PIRE_EXTRA_CAPTURE_H

/*
 * Batched Runner over a Pire::SlowScanner (scanners/slow.h): Matches(sc, str) per string, i.e.
 * Final(Runner(sc).Begin().Run(str).End().State()).
 *
 * Which strings matched -- or, inverted, did not -- answered on the device (pire_hip_slow_run_select): the scan and the hit
 * list behind one call, Begin() and End() around every string as in Matches():
 *     run.Run(text, offsets, n).Select();          run.Run(strings).Select(true);      // true: grep -v
 *     run.Hits()       ascending indices of the selected strings          run.HitCount()  how many
 * A buffer as it was read, cut into lines, scanned and selected on the device (pire_hip_slow_lines_select / _gather; getline's
 * semantics, as BatchRunner::RunLines()):
 *     run.RunLines(raw, size);                     run.RunLines(raw, size, '\n', true);
 *     run.HitSpans()   [2 * k], [2 * k + 1]: hit k is raw[begin, end)      run.LineCount()  lines in the buffer
 *     run.HitText()    the selected lines back to back, '\n' (or the byte given) behind each: grep's output -- inverted: grep
 *                      -v's --, gathered on the device               run.HitTextOffsets()  hit k is HitText()[o[k], o[k + 1])
 * The caller's arrays are read when an accessor first asks: they live until then.  HitText() is a call of its own, as in
 * BatchRunner: after Hits() / HitSpans() it scans the buffer a second time.
 */
class SlowBatchRunner {
public:
	explicit SlowBatchRunner(const Pire::SlowScanner& sc)
	    : m_table(nullptr), m_form(kNone), m_text(nullptr), m_offsets(nullptr), m_n(0), m_len(0), m_delim('\n'), m_invert(false),
	      m_listed(false), m_haveText(false), m_textTail('\n'), m_hitCount(0), m_lineCount(0)
	{
		const std::string blob = SavedBlob(sc);
		Check(pire_hip_slow_table_create(blob.data(), blob.size(), &m_table));
	}
	~SlowBatchRunner() { pire_hip_slow_table_destroy(m_table); }

	/* Begin().Run().End() for n strings; returns operator bool of the reference's RunHelper per string. */
	std::vector<char> Matches(const char* text, const uint64_t* offsets, size_t n)
	{
		std::vector<uint8_t> fin(n);
		Check(pire_hip_slow_run(m_table, text, OwnedStrings::OffsetsOr(offsets, n), n, PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END,
		                        fin.data(), nullptr, nullptr, nullptr));
		return std::vector<char>(fin.begin(), fin.end());
	}

	/* The batch of the hit forms: string i = text[offsets[i], offsets[i+1]).  Host pointers. */
	SlowBatchRunner& Run(const char* text, const uint64_t* offsets, size_t n) { return SetBatch(kStrings, text, offsets, n, 0, '\n', false); }
	SlowBatchRunner& Run(const std::vector<ystring>& strings)
	{
		m_ownStrings.Assign(strings);
		return Run(m_ownStrings.Text(), m_ownStrings.Offsets(), strings.size());
	}
	SlowBatchRunner& Select(bool invert = false)
	{
		m_invert = invert;
		m_listed = m_haveText = false;
		m_context.NewSelection();
		m_files.NewSelection();
		return *this;
	}
	SlowBatchRunner& RunLines(const char* raw, size_t size, char delim = '\n', bool invert = false)
	{
		return SetBatch(kLines, raw, nullptr, 0, size, delim, invert);
	}
	uint64_t HitCount() { FetchHits(); return m_hitCount; }
	const std::vector<uint64_t>& Hits() { FetchHits(); return m_hits; }
	uint64_t LineCount() { NeedLines("LineCount()"); FetchHits(); return m_lineCount; }
	const std::vector<uint64_t>& HitSpans() { NeedLines("HitSpans()"); FetchHits(); return m_hitSpans; }
	const std::string& HitText(char tail = '\n') { FetchHitText(tail); return m_hitText; }
	const std::vector<uint64_t>& HitTextOffsets()
	{
		if (!m_haveText)
			FetchHitText('\n');
		return m_hitTextOffsets;
	}
	/* The hits of RunLines() by file (pire_hip_slow_lines_files_select): BatchRunner::Files() and its accessors.  It honours
	 * Select(invert): grep -v -c, grep -v -l. */
	SlowBatchRunner& Files(const std::vector<uint64_t>& fileBytes)
	{
		NeedLines("Files()");
		m_files.Ask(fileBytes);
		return *this;
	}
	const std::vector<uint64_t>& FileHitCounts() { FetchFiles("FileHitCounts()"); return m_files.Counts(); }
	const std::vector<uint64_t>& FilesWithHits() { FetchFiles("FilesWithHits()"); return m_files.With(); }
	const std::vector<uint64_t>& FilesWithoutHits() { FetchFilesWithout("FilesWithoutHits()"); return m_files.Without(); }
	const std::vector<uint64_t>& HitFiles() { FetchFiles("HitFiles()"); return m_files.HitFile(); }
	const std::vector<uint64_t>& HitFileLines() { FetchFiles("HitFileLines()"); return m_files.HitLine(); }
	const std::vector<uint64_t>& FileLines() { FetchFiles("FileLines()"); return m_files.FileLines(); }
	uint64_t Straddles() { FetchFiles("Straddles()"); return m_files.Straddles(); }

	/* The hits of RunLines() -- inverted: the lines that did not match, grep -v -C -- and the lines around them
	 * (pire_hip_slow_lines_context_select / _gather): BatchRunner::Context() and its accessors.  It honours Select(invert). */
	SlowBatchRunner& Context(uint64_t before, uint64_t after)
	{
		NeedLines("Context()");
		m_context.Ask(before, after);
		return *this;
	}
	const std::vector<uint64_t>& ContextLines() { FetchContext("ContextLines()"); return m_context.Lines(); }
	const std::vector<uint8_t>& ContextFlags() { FetchContext("ContextFlags()"); return m_context.Flags(); }
	const std::vector<uint64_t>& ContextSpans() { FetchContext("ContextSpans()"); return m_context.Spans(); }
	uint64_t ContextGroupCount() { FetchContext("ContextGroupCount()"); return m_context.GroupCount(); }
	const std::string& ContextText(char tail = '\n') { FetchContextText("ContextText()", tail); return m_context.Text(); }
	const std::vector<uint64_t>& ContextTextOffsets()
	{
		if (!m_context.HasText())
			FetchContextText("ContextTextOffsets()", '\n');
		return m_context.TextOffsets();
	}

private:
	SlowBatchRunner(const SlowBatchRunner&);
	SlowBatchRunner& operator=(const SlowBatchRunner&);

	enum Form { kNone, kStrings, kLines };
	SlowBatchRunner& SetBatch(Form form, const char* text, const uint64_t* offsets, size_t n, size_t len, char delim, bool invert)
	{
		m_form = form, m_text = text, m_offsets = offsets, m_n = n, m_len = len, m_delim = uint8_t(delim), m_invert = invert;
		m_listed = m_haveText = false;
		m_context.NewBatch();
		m_files.NewBatch();
		return *this;
	}
	uint32_t Mode() const { return m_invert ? PIRE_HIP_FINAL_SELECT_ZERO : 0; }
	void NeedLines(const char* what) const
	{
		if (m_form != kLines)
			throw Pire::Error(std::string("pire_hip: ") + what + " follows RunLines()");
	}

	/* One call with room for every string -- RunLines(): for a hit on every line of 64 bytes or more, BatchRunner's first
	 * capacity --, and a second one where there are more */
	void FetchHits()
	{
		if (m_listed)
			return;
		if (m_form == kNone)
			throw Pire::Error("pire_hip: Hits() follows Run() or RunLines()");
		const uint32_t flags = PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END;
		GrowAndRetry(m_form == kLines ? m_len / 64 + 1024 : m_n, [&](size_t cap) {
			m_hits.resize(cap);
			m_hitSpans.resize(m_form == kLines ? cap * 2 : 0);
			Check(m_form == kLines
			          ? pire_hip_slow_lines_select(m_table, m_text, m_len, m_delim, flags, Mode(), &m_lineCount, m_hits.data(),
			                                       m_hitSpans.data(), cap, &m_hitCount, nullptr)
			          : pire_hip_slow_run_select(m_table, m_text, OwnedStrings::OffsetsOr(m_offsets, m_n), m_n, flags, Mode(), nullptr, nullptr,
			                                     nullptr, m_hits.data(), cap, &m_hitCount, nullptr));
			return size_t(m_hitCount);
		});
		m_hits.resize(m_hitCount);
		m_hitSpans.resize(m_form == kLines ? m_hitCount * 2 : 0);
		m_listed = true;
	}

	/* RunLines(): the selected lines as bytes; room for every byte they can have, and for the hits that are known, or else
	 * FetchHits()'s */
	void FetchHitText(char tail)
	{
		NeedLines("HitText()");
		if (m_haveText && m_textTail == tail)
			return;
		uint64_t count = 0, bytes = 0;
		GrowAndRetry(m_listed ? size_t(m_hitCount) : m_len / 64 + 1024, [&](size_t cap) {
			m_hitTextOffsets.resize(cap + 1);
			m_hitText.resize(m_len + cap + 1);
			Check(pire_hip_slow_lines_gather(m_table, m_text, m_len, m_delim, PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END, Mode(), uint8_t(tail),
			                                 &m_lineCount, nullptr, cap, &count, &m_hitText[0], m_hitText.size(), m_hitTextOffsets.data(),
			                                 &bytes, nullptr));
			return size_t(count);   // (the text has room for the whole buffer and a tail per hit: where the hits fit, the bytes do)
		});
		m_hitText.resize(bytes);
		m_hitTextOffsets.resize(count + 1);
		m_textTail = tail;
		m_haveText = true;
	}

	/* Context(): the C call of a LineContext::Call, on this runner's table, buffer and selection */
	void ContextCall(const LineContext::Call& c)
	{
		const uint32_t flags = PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END;
		Check(c.gather ? pire_hip_slow_lines_context_gather(m_table, m_text, m_len, m_delim, flags, Mode(), c.before, c.after, c.lineCount, c.lines,
		                                                    c.flags, c.spans, c.cap, c.selCount, c.groupCount, c.hitCount, c.tail, c.text,
		                                                    c.textCap, c.offsets, c.bytes, nullptr)
		               : pire_hip_slow_lines_context_select(m_table, m_text, m_len, m_delim, flags, Mode(), c.before, c.after, c.lineCount, c.lines,
		                                                    c.flags, c.spans, c.cap, c.selCount, c.groupCount, c.hitCount, nullptr));
	}
	/* Files(): the C call of a LineFiles::Call, on this runner's table, buffer and selection */
	void FilesCall(const LineFiles::Call& c)
	{
		Check(pire_hip_slow_lines_files_select(m_table, m_text, m_len, m_delim, PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END, Mode(), c.fileBytes,
		                                       c.files, c.fileMode, c.lineCount, c.hits, c.spans, c.hitFile, c.hitLine, c.cap, c.hitCount,
		                                       c.fileLines, c.fileFirst, c.outFiles, c.fileCap, c.fileCount, c.straddles, nullptr));
	}
	void FetchFiles(const char* what) { m_files.FetchLists(what, m_len, [&](const LineFiles::Call& c) { FilesCall(c); }); }
	void FetchFilesWithout(const char* what) { m_files.FetchWithout(what, [&](const LineFiles::Call& c) { FilesCall(c); }); }
	void FetchContext(const char* what) { m_context.FetchLists(what, m_len, [&](const LineContext::Call& c) { ContextCall(c); }); }
	void FetchContextText(const char* what, char tail)
	{
		m_context.FetchText(what, m_len, tail, [&](const LineContext::Call& c) { ContextCall(c); });
	}

	pire_hip_slow_table* m_table;
	Form m_form;
	const char* m_text;           // Run(): the strings' text; RunLines(): the raw buffer of m_len bytes
	const uint64_t* m_offsets;
	size_t m_n, m_len;
	uint8_t m_delim;
	bool m_invert;
	bool m_listed, m_haveText;    // m_hits (and m_hitSpans, m_lineCount) / m_hitText are the batch's, with the tail m_textTail
	char m_textTail;
	OwnedStrings m_ownStrings;
	uint64_t m_hitCount, m_lineCount;
	std::vector<uint64_t> m_hits, m_hitSpans, m_hitTextOffsets;
	std::string m_hitText;
	LineContext m_context;        // Context(): the request and what was fetched for it
	LineFiles m_files;            // Files(): the request and what was fetched for it
};

/*
 * easy.h's choice, made for the caller: Pire::Regexp (easy.h:211-214) compiles a Scanner where Fsm::Determine() succeeds and
 * falls back to a SlowScanner where it gives up (fsm.cpp: more than 200 000 states -- a pattern like x.{40}$), and its user
 * never learns which.  LineMatcher does the same for a buffer of lines: constructed from the Fsm as the caller built it
 * (surrounded or not: PrependAnything() / AppendAnything() are the caller's), it offers one surface over
 * BatchRunner<Scanner>::RunLines() and SlowBatchRunner::RunLines():
 *     Pire::Hip::LineMatcher grep(fsm);
 *     grep.RunLines(raw, size);                    grep.RunLines(raw, size, '\n', true);     // true: grep -v, slow form only
 *     grep.HitText()   grep.HitSpans()   grep.Hits()   grep.HitCount()   grep.LineCount()   grep.IsSlow()
 * Begin() and End() are stepped around every line, as Matches() does.  The inverted selection exists for the SlowScanner
 * alone (the library has none behind pire_hip_select): RunLines(.., true) on a determinised pattern throws.
 */
class LineMatcher {
public:
	explicit LineMatcher(Pire::Fsm fsm)
	    : m_fast(nullptr), m_slow(nullptr)
	{
		if (fsm.Determine()) {
			m_scanner = fsm.Compile<Pire::Scanner>();
			m_fast = new BatchRunner<Pire::Scanner>(m_scanner);
		} else {
			m_slowScanner = fsm.Compile<Pire::SlowScanner>();
			m_slow = new SlowBatchRunner(m_slowScanner);
		}
	}
	~LineMatcher()
	{
		delete m_fast;
		delete m_slow;
	}
	bool IsSlow() const { return m_slow != nullptr; }
	LineMatcher& RunLines(const char* raw, size_t size, char delim = '\n', bool invert = false)
	{
		if (m_slow)
			m_slow->RunLines(raw, size, delim, invert);
		else if (invert)
			throw Pire::Error("pire_hip: LineMatcher::RunLines(): the inverted selection follows a SlowScanner only");
		else
			m_fast->Begin().RunLines(raw, size, delim).End();
		return *this;
	}
	uint64_t LineCount() { return m_slow ? m_slow->LineCount() : m_fast->LineCount(); }
	uint64_t HitCount() { return m_slow ? m_slow->HitCount() : m_fast->HitCount(); }
	const std::vector<uint64_t>& Hits() { return m_slow ? m_slow->Hits() : m_fast->Hits(); }
	const std::vector<uint64_t>& HitSpans() { return m_slow ? m_slow->HitSpans() : m_fast->HitSpans(); }
	const std::string& HitText(char tail = '\n') { return m_slow ? m_slow->HitText(tail) : m_fast->HitText(tail); }
	const std::vector<uint64_t>& HitTextOffsets() { return m_slow ? m_slow->HitTextOffsets() : m_fast->HitTextOffsets(); }
	/* Context() and its accessors, forwarded to whichever runner the pattern picked */
	LineMatcher& Context(uint64_t before, uint64_t after)
	{
		if (m_slow)
			m_slow->Context(before, after);
		else
			m_fast->Context(before, after);
		return *this;
	}
	const std::vector<uint64_t>& ContextLines() { return m_slow ? m_slow->ContextLines() : m_fast->ContextLines(); }
	const std::vector<uint8_t>& ContextFlags() { return m_slow ? m_slow->ContextFlags() : m_fast->ContextFlags(); }
	const std::vector<uint64_t>& ContextSpans() { return m_slow ? m_slow->ContextSpans() : m_fast->ContextSpans(); }
	uint64_t ContextGroupCount() { return m_slow ? m_slow->ContextGroupCount() : m_fast->ContextGroupCount(); }
	const std::string& ContextText(char tail = '\n') { return m_slow ? m_slow->ContextText(tail) : m_fast->ContextText(tail); }
	const std::vector<uint64_t>& ContextTextOffsets() { return m_slow ? m_slow->ContextTextOffsets() : m_fast->ContextTextOffsets(); }
	/* Files() and its accessors, forwarded to whichever runner the pattern picked */
	LineMatcher& Files(const std::vector<uint64_t>& fileBytes)
	{
		if (m_slow)
			m_slow->Files(fileBytes);
		else
			m_fast->Files(fileBytes);
		return *this;
	}
	const std::vector<uint64_t>& FileHitCounts() { return m_slow ? m_slow->FileHitCounts() : m_fast->FileHitCounts(); }
	const std::vector<uint64_t>& FilesWithHits() { return m_slow ? m_slow->FilesWithHits() : m_fast->FilesWithHits(); }
	const std::vector<uint64_t>& FilesWithoutHits() { return m_slow ? m_slow->FilesWithoutHits() : m_fast->FilesWithoutHits(); }
	const std::vector<uint64_t>& HitFiles() { return m_slow ? m_slow->HitFiles() : m_fast->HitFiles(); }
	const std::vector<uint64_t>& HitFileLines() { return m_slow ? m_slow->HitFileLines() : m_fast->HitFileLines(); }
	const std::vector<uint64_t>& FileLines() { return m_slow ? m_slow->FileLines() : m_fast->FileLines(); }
	uint64_t Straddles() { return m_slow ? m_slow->Straddles() : m_fast->Straddles(); }

private:
	LineMatcher(const LineMatcher&);
	LineMatcher& operator=(const LineMatcher&);
	Pire::Scanner m_scanner;           // the one the pattern compiled to; the runners read it
	Pire::SlowScanner m_slowScanner;
	BatchRunner<Pire::Scanner>* m_fast;
	SlowBatchRunner* m_slow;
};

/*
 * Truth tables of a LineQuery over k terms (include/pire_hip.h, pire_hip_combine): bit m of the table says whether a line is
 * selected whose member mask is m -- bit j of m: term j lists the line.  k is 1 .. PIRE_HIP_COMBINE_MAX_LISTS.
 *     Truth::All(2)                                   both terms                     Truth::Any(3)   at least one of three
 *     Truth::Of(2, [](unsigned m) { return m == 1; }) the first and not the second   (grep a | grep -v b)
 */
struct Truth {
	template <class Predicate>
	static uint64_t Of(unsigned k, Predicate selected)
	{
		if (k < 1 || k > PIRE_HIP_COMBINE_MAX_LISTS)
			throw Pire::Error("pire_hip: Truth: 1 .. 6 terms");
		uint64_t table = 0;
		for (unsigned m = 0; m < (1u << k); ++m)
			if (selected(m))
				table |= uint64_t(1) << m;
		return table;
	}
	static uint64_t All(unsigned k)
	{
		return Of(k, [k](unsigned m) { return m == (1u << k) - 1; });
	}
	static uint64_t Any(unsigned k)
	{
		return Of(k, [](unsigned m) { return m != 0; });
	}
};

/*
 * Several scanners over the lines of one buffer, and a boolean function of what they match: one call, one split, one wait
 * (pire_hip_lines_combine_select / _gather).  Begin() and End() are stepped around every line -- or column -- of every term, as
 * Matches() does.
 *     Pire::Hip::LineQuery q;
 *     q.Add(errors).AddSlow(noise, true);                              // term 0: a Scanner; term 1: the lines a SlowScanner does NOT match
 *     q.AddField(user, 2);                                             // term 2: a Scanner on column 2 of the line (0-based, '\t' between)
 *     q.Where(Pire::Hip::Truth::All(3)).RunLines(raw, size);           // Where() is optional: every term
 *     q.Hits()  q.HitSpans()  q.HitMembers()  q.HitCount()  q.LineCount()  q.TermCounts()  q.HitText()  q.HitTextOffsets()
 * HitMembers()[r] is the member mask of Hits()[r]; TermCounts()[j] is grep -c of term j alone.  The scanners are read when they
 * are added; the buffer is read when an accessor first asks: it lives until then.  HitText() is a call of its own, as in
 * BatchRunner: after Hits() it scans the buffer a second time.  A Scanner term lists the lines whose end state is Final.
 */
class LineQuery {
public:
	LineQuery() : m_truth(0), m_where(false), m_ran(false), m_raw(nullptr), m_len(0), m_delim('\n'), m_listed(false), m_haveText(false),
	              m_textTail('\n'), m_lineCount(0), m_hitCount(0) {}
	~LineQuery()
	{
		for (size_t j = 0; j < m_terms.size(); ++j) {
			pire_hip_table_destroy(m_terms[j].table);
			pire_hip_slow_table_destroy(m_terms[j].slow_table);
		}
	}
	LineQuery& Add(const Pire::Scanner& sc) { return AddTerm(&sc, nullptr, false, PIRE_HIP_TERM_LINE, 0, false); }
	LineQuery& AddField(const Pire::Scanner& sc, uint32_t field, char sep = '\t', bool rest = false)
	{
		return AddTerm(&sc, nullptr, false, field, uint8_t(sep), rest);
	}
	LineQuery& AddSlow(const Pire::SlowScanner& sc, bool invert = false) { return AddTerm(nullptr, &sc, invert, PIRE_HIP_TERM_LINE, 0, false); }
	LineQuery& Where(uint64_t truth)
	{
		m_truth = truth, m_where = true;
		m_listed = m_haveText = false;
		return *this;
	}
	LineQuery& RunLines(const char* raw, size_t size, char delim = '\n')
	{
		m_raw = raw, m_len = size, m_delim = delim, m_ran = true;
		m_listed = m_haveText = false;
		return *this;
	}
	size_t Terms() const { return m_terms.size(); }
	uint64_t LineCount() { FetchLists("LineCount()"); return m_lineCount; }
	uint64_t HitCount() { FetchLists("HitCount()"); return m_hitCount; }
	const std::vector<uint64_t>& Hits() { FetchLists("Hits()"); return m_hits; }
	const std::vector<uint64_t>& HitSpans() { FetchLists("HitSpans()"); return m_hitSpans; }
	const std::vector<uint8_t>& HitMembers() { FetchLists("HitMembers()"); return m_hitMembers; }
	const std::vector<uint64_t>& TermCounts() { FetchLists("TermCounts()"); return m_termCounts; }
	const std::string& HitText(char tail = '\n') { FetchText("HitText()", tail); return m_hitText; }
	const std::vector<uint64_t>& HitTextOffsets()
	{
		if (!m_haveText)
			FetchText("HitTextOffsets()", '\n');
		return m_hitTextOffsets;
	}

private:
	LineQuery(const LineQuery&);
	LineQuery& operator=(const LineQuery&);
	LineQuery& AddTerm(const Pire::Scanner* fast, const Pire::SlowScanner* slow, bool invert, uint32_t column, uint32_t sep, bool rest)
	{
		pire_hip_line_term t = {};
		const std::string blob = fast ? SavedBlob(*fast) : SavedBlob(*slow);
		if (fast)
			Check(pire_hip_table_create(blob.data(), blob.size(), &t.table));
		else
			Check(pire_hip_slow_table_create(blob.data(), blob.size(), &t.slow_table));
		t.mode = invert ? PIRE_HIP_FINAL_SELECT_ZERO : 0;
		t.run_flags = PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END;
		t.column = column, t.sep = sep, t.field_mode = rest ? PIRE_HIP_FIELDS_REST : 0;
		m_terms.push_back(t);
		m_listed = m_haveText = false;
		return *this;
	}
	void Need(const char* what) const
	{
		if (!m_ran)
			throw Pire::Error(std::string("pire_hip: ") + what + " follows RunLines()");
	}
	/* Where() was not called: every term.  (More terms than a table has bits for: the library refuses the call.) */
	uint64_t TruthTable() const
	{
		const size_t k = m_terms.size();
		return m_where ? m_truth : k >= 1 && k <= PIRE_HIP_COMBINE_MAX_LISTS ? Truth::All(unsigned(k)) : 0;
	}
	/* One call with room for a hit per 64 bytes of the buffer, and a second one where there are more */
	void FetchLists(const char* what)
	{
		Need(what);
		if (m_listed)
			return;
		m_termCounts.assign(m_terms.size(), 0);
		GrowAndRetry(m_len / 64 + 1024, [&](size_t cap) {
			m_hits.resize(cap);
			m_hitSpans.resize(cap * 2);
			m_hitMembers.resize(cap);
			Check(pire_hip_lines_combine_select(m_terms.data(), uint32_t(m_terms.size()), TruthTable(), m_raw, m_len, uint8_t(m_delim), 0,
			                                    &m_lineCount, m_hits.data(), m_hitSpans.data(), m_hitMembers.data(), cap, &m_hitCount,
			                                    m_termCounts.data(), nullptr));
			return size_t(m_hitCount);
		});
		m_hits.resize(m_hitCount);
		m_hitSpans.resize(m_hitCount * 2);
		m_hitMembers.resize(m_hitCount);
		m_listed = true;
	}
	/* The selected lines as bytes; room for every byte they can have, and for the hits that are known, or else FetchLists()'s */
	void FetchText(const char* what, char tail)
	{
		Need(what);
		if (m_haveText && m_textTail == tail)
			return;
		uint64_t lines = 0, count = 0, bytes = 0;
		GrowAndRetry(m_listed ? size_t(m_hitCount) : m_len / 64 + 1024, [&](size_t cap) {
			m_hitTextOffsets.resize(cap + 1);
			m_hitText.resize(m_len + cap + 1);
			Check(pire_hip_lines_combine_gather(m_terms.data(), uint32_t(m_terms.size()), TruthTable(), m_raw, m_len, uint8_t(m_delim), 0, &lines,
			                                    nullptr, nullptr, nullptr, cap, &count, nullptr, uint8_t(tail), &m_hitText[0], m_hitText.size(),
			                                    m_hitTextOffsets.data(), &bytes, nullptr));
			return size_t(count);   // (the text has room for the whole buffer and a tail per line: where the hits fit, the bytes do)
		});
		m_hitText.resize(bytes);
		m_hitTextOffsets.resize(count + 1);
		m_textTail = tail;
		m_haveText = true;
	}
	std::vector<pire_hip_line_term> m_terms;
	uint64_t m_truth;
	bool m_where, m_ran;
	const char* m_raw;
	size_t m_len;
	char m_delim;
	bool m_listed, m_haveText;
	char m_textTail;
	uint64_t m_lineCount, m_hitCount;
	std::vector<uint64_t> m_hits, m_hitSpans, m_termCounts, m_hitTextOffsets;
	std::vector<uint8_t> m_hitMembers;
	std::string m_hitText;
};

/*
 * Where the text lies: Pire::LongestPrefix / ShortestPrefix of a head scanner and Pire::LongestSuffix / ShortestSuffix of a tail
 * scanner (run.h:277-362; the tail scanner compiled from Fsm::Reverse(), pire_ut.cpp:283) over n strings, and the byte ranges
 * they mean, on the device (include/pire_hip.h, "the matched heads and tails, on the device").  Either scanner may be absent
 * (a null pointer), not both; the options are PIRE_HIP_AFFIX_* bits.  A string is selected when every scanner that is given
 * accepts a prefix (suffix) of it -- the empty one counts.
 *     Pire::Hip::AffixBatchRunner<Pire::Scanner> trim(&blanks, &blanksReversed);
 *     trim.Run(text, offsets, n).Select(PIRE_HIP_AFFIX_REST);      trim.Run(strings).Select(PIRE_HIP_AFFIX_HEAD);
 *     trim.Hits()      ascending indices of the selected strings           trim.HitCount()  how many
 *     trim.Spans()     [2 * k], [2 * k + 1]: the part of hit k is text[begin, end)
 * A buffer as it was read, cut into lines on the device (pire_hip_affix_lines_gather; getline's semantics, as
 * BatchRunner::RunLines()): `grep -o '^re'` (HEAD), `sed 's/^re//'` on the lines that match (REST), a trim of both ends (REST
 * with both scanners):
 *     trim.RunLines(raw, size, '\n', PIRE_HIP_AFFIX_REST);
 *     trim.Spans()     byte ranges of raw                                  trim.LineCount()  lines in the buffer
 *     trim.HitText()   the parts back to back, '\n' (or the byte given) behind each, gathered on the device
 *     trim.HitTextOffsets()   part k is HitText()[o[k], o[k + 1])
 * The caller's arrays are read when an accessor first asks: they live until then.  HitText() is a call of its own, as in
 * BatchRunner: after Hits() / Spans() it scans the buffer a second time.
 */
template <class Scanner>
class AffixBatchRunner {
public:
	AffixBatchRunner(const Scanner* head, const Scanner* tail, uint32_t headOpts = PIRE_HIP_AFFIX_LONGEST,
	                 uint32_t tailOpts = PIRE_HIP_AFFIX_LONGEST)
	    : m_head(head ? new Table<Scanner>(*head) : nullptr), m_tail(nullptr), m_headOpts(headOpts), m_tailOpts(tailOpts), m_form(kNone),
	      m_text(nullptr), m_offsets(nullptr), m_n(0), m_len(0), m_delim('\n'), m_part(PIRE_HIP_AFFIX_HEAD), m_listed(false), m_haveText(false),
	      m_textTail('\n'), m_hitCount(0), m_lineCount(0)
	{
		try {
			m_tail = tail ? new Table<Scanner>(*tail) : nullptr;
		} catch (...) {
			delete m_head;
			throw;
		}
	}
	~AffixBatchRunner()
	{
		delete m_head;
		delete m_tail;
	}

	/* The batch: string i = text[offsets[i], offsets[i+1]).  Host pointers. */
	AffixBatchRunner& Run(const char* text, const uint64_t* offsets, size_t n) { return SetBatch(kStrings, text, offsets, n, 0, '\n', m_part); }
	AffixBatchRunner& Run(const std::vector<ystring>& strings)
	{
		m_ownStrings.Assign(strings);
		return Run(m_ownStrings.Text(), m_ownStrings.Offsets(), strings.size());
	}
	AffixBatchRunner& Select(uint32_t part)
	{
		m_part = part;
		m_listed = m_haveText = false;
		return *this;
	}
	AffixBatchRunner& RunLines(const char* raw, size_t size, char delim = '\n', uint32_t part = PIRE_HIP_AFFIX_HEAD)
	{
		return SetBatch(kLines, raw, nullptr, 0, size, delim, part);
	}
	uint64_t HitCount() { FetchHits(); return m_hitCount; }
	const std::vector<uint64_t>& Hits() { FetchHits(); return m_hits; }
	const std::vector<uint64_t>& Spans() { FetchHits(); return m_spans; }
	uint64_t LineCount() { NeedLines("LineCount()"); FetchHits(); return m_lineCount; }
	const std::string& HitText(char tail = '\n') { FetchHitText(tail); return m_hitText; }
	const std::vector<uint64_t>& HitTextOffsets()
	{
		if (!m_haveText)
			FetchHitText('\n');
		return m_hitTextOffsets;
	}

private:
	AffixBatchRunner(const AffixBatchRunner&);
	AffixBatchRunner& operator=(const AffixBatchRunner&);

	enum Form { kNone, kStrings, kLines };
	AffixBatchRunner& SetBatch(Form form, const char* text, const uint64_t* offsets, size_t n, size_t len, char delim, uint32_t part)
	{
		m_form = form, m_text = text, m_offsets = offsets, m_n = n, m_len = len, m_delim = uint8_t(delim), m_part = part;
		m_listed = m_haveText = false;
		return *this;
	}
	pire_hip_table* Head() const { return m_head ? m_head->Handle() : nullptr; }
	pire_hip_table* Tail() const { return m_tail ? m_tail->Handle() : nullptr; }
	void NeedLines(const char* what) const
	{
		if (m_form != kLines)
			throw Pire::Error(std::string("pire_hip: ") + what + " follows RunLines()");
	}

	/* One call with room for every string -- RunLines(): for a hit on every line of 64 bytes or more, BatchRunner's first
	 * capacity --, and a second one where there are more */
	void FetchHits()
	{
		if (m_listed)
			return;
		if (m_form == kNone)
			throw Pire::Error("pire_hip: Hits() follows Run() or RunLines()");
		GrowAndRetry(m_form == kLines ? m_len / 64 + 1024 : m_n, [&](size_t cap) {
			m_hits.resize(cap);
			m_spans.resize(cap * 2);
			Check(m_form == kLines
			          ? pire_hip_affix_lines_gather(Head(), m_headOpts, Tail(), m_tailOpts, m_text, m_len, m_delim, m_part, 0,
			                                        PIRE_HIP_GATHER_NO_TAIL, &m_lineCount, m_hits.data(), m_spans.data(), cap, &m_hitCount,
			                                        nullptr, 0, nullptr, nullptr, nullptr)
			          : pire_hip_affix_run_select(Head(), m_headOpts, Tail(), m_tailOpts, m_text, OwnedStrings::OffsetsOr(m_offsets, m_n), m_n,
			                                      m_part, 0, nullptr, nullptr, m_hits.data(), m_spans.data(), cap, &m_hitCount, nullptr));
			return size_t(m_hitCount);
		});
		m_hits.resize(m_hitCount);
		m_spans.resize(m_hitCount * 2);
		m_listed = true;
	}

	/* RunLines(): the parts as bytes; room for every byte they can have, and for the hits that are known, or else FetchHits()'s */
	void FetchHitText(char tail)
	{
		NeedLines("HitText()");
		if (m_haveText && m_textTail == tail)
			return;
		uint64_t count = 0, bytes = 0;
		GrowAndRetry(m_listed ? size_t(m_hitCount) : m_len / 64 + 1024, [&](size_t cap) {
			m_hitTextOffsets.resize(cap + 1);
			m_hitText.resize(m_len + cap + 1);
			Check(pire_hip_affix_lines_gather(Head(), m_headOpts, Tail(), m_tailOpts, m_text, m_len, m_delim, m_part, 0, uint8_t(tail),
			                                  &m_lineCount, nullptr, nullptr, cap, &count, &m_hitText[0], m_hitText.size(),
			                                  m_hitTextOffsets.data(), &bytes, nullptr));
			return size_t(count);   // (the text has room for the whole buffer and a tail per hit: where the hits fit, the bytes do)
		});
		m_hitText.resize(bytes);
		m_hitTextOffsets.resize(count + 1);
		m_textTail = tail;
		m_haveText = true;
	}

	Table<Scanner>* m_head;       // nullable: no head is looked for
	Table<Scanner>* m_tail;       // nullable
	uint32_t m_headOpts, m_tailOpts;
	Form m_form;
	const char* m_text;           // Run(): the strings' text; RunLines(): the raw buffer of m_len bytes
	const uint64_t* m_offsets;
	size_t m_n, m_len;
	uint8_t m_delim;
	uint32_t m_part;
	bool m_listed, m_haveText;    // m_hits, m_spans (and m_lineCount) / m_hitText are the batch's, with the tail m_textTail
	char m_textTail;
	OwnedStrings m_ownStrings;
	uint64_t m_hitCount, m_lineCount;
	std::vector<uint64_t> m_hits, m_spans, m_hitTextOffsets;
	std::string m_hitText;
};

/*
 * Where the leftmost-longest match lies: Pire::LongestSuffix (run.h:313-341) through a scanner compiled from Fsm::Reverse() of
 * `re` followed by anything, then Pire::LongestPrefix (run.h:277-311; ShortestPrefix with PIRE_HIP_SEARCH_SHORTEST) through the
 * scanner of `re` from where the first search ended -- on the device, both in one launch (include/pire_hip.h, "where the match
 * lies").  Neither scanner is Surround()ed; the options are PIRE_HIP_SEARCH_* bits.
 *     Pire::Hip::SearchBatchRunner<Pire::Scanner> find(reversedTail, forward);
 *     find.Run(text, offsets, n);      find.Run(strings);
 *     find.Select();   (optional: Run() alone is enough)
 *     find.Hits()      ascending indices of the strings with a match       find.HitCount()  how many
 *     find.Spans()     [2 * k], [2 * k + 1]: the match of hit k is text[begin, end)
 * A buffer as it was read, cut into lines on the device (pire_hip_search_lines_gather; getline's semantics, as
 * BatchRunner::RunLines()): `grep -o` for the first match of each line:
 *     find.RunLines(raw, size, '\n');
 *     find.Spans()     byte ranges of raw                                  find.LineCount()  lines in the buffer
 *     find.HitText()   the matches back to back, '\n' (or the byte given) behind each, gathered on the device
 *     find.HitTextOffsets()   match k is HitText()[o[k], o[k + 1])
 * EVERY match of every string (line), not the first alone (pire_hip_search_all / pire_hip_search_all_lines_gather; an empty
 * match is never reported): All() behind Run() or RunLines() -- with RunLines() and '\n', `grep -o`'s output:
 *     find.Run(strings).All();
 *     find.Hits()      the string of match k: ascending, with repeats       find.HitCount()  matches
 *     find.Spans()     as above, one pair per match                         find.Rows()      [n + 1]: the matches of string i are
 *                                                                                            entries [rows[i], rows[i+1]); Run() only
 *     find.RunLines(raw, size).All().HitText();
 * Select() switches back to the first match, which is what a new batch starts with.
 * The caller's arrays are read when an accessor first asks: they live until then.  HitText() is a call of its own, as in
 * BatchRunner: after Hits() / Spans() it scans the buffer a second time.
 */
template <class Scanner>
class SearchBatchRunner {
public:
	SearchBatchRunner(const Scanner& reversedTail, const Scanner& forward, uint32_t opts = 0)
	    : m_rev(reversedTail), m_fwd(forward), m_opts(opts), m_form(kNone), m_text(nullptr), m_offsets(nullptr), m_n(0), m_len(0), m_delim('\n'),
	      m_fetchAll(nullptr), m_linesCall(pire_hip_search_lines_gather), m_listed(false), m_haveText(false), m_textTail('\n'), m_hitCount(0), m_lineCount(0)
	{
	}

	/* The batch: string i = text[offsets[i], offsets[i+1]).  Host pointers. */
	SearchBatchRunner& Run(const char* text, const uint64_t* offsets, size_t n) { return SetBatch(kStrings, text, offsets, n, 0, '\n'); }
	SearchBatchRunner& Run(const std::vector<ystring>& strings)
	{
		m_ownStrings.Assign(strings);
		return Run(m_ownStrings.Text(), m_ownStrings.Offsets(), strings.size());
	}
	/* the strings with a match and where it lies: what Hits() / Spans() answer (there is one selection; the call is AffixBatchRunner's idiom) */
	SearchBatchRunner& Select() { return SetAll(nullptr, pire_hip_search_lines_gather); }
	/* every match of every string (line): Hits() answers the owners, one entry per match */
	SearchBatchRunner& All() { return SetAll(&SearchBatchRunner::FetchAll, pire_hip_search_all_lines_gather); }
	SearchBatchRunner& RunLines(const char* raw, size_t size, char delim = '\n') { return SetBatch(kLines, raw, nullptr, 0, size, delim); }
	uint64_t HitCount() { FetchHits(); return m_hitCount; }
	const std::vector<uint64_t>& Hits() { FetchHits(); return m_hits; }
	const std::vector<uint64_t>& Spans() { FetchHits(); return m_spans; }
	uint64_t LineCount() { NeedLines("LineCount()"); FetchHits(); return m_lineCount; }
	const std::string& HitText(char tail = '\n') { FetchHitText(tail); return m_hitText; }
	const std::vector<uint64_t>& HitTextOffsets()
	{
		if (!m_haveText)
			FetchHitText('\n');
		return m_hitTextOffsets;
	}
	/* All() behind Run(): n + 1 row starts into Hits() / Spans() */
	const std::vector<uint64_t>& Rows()
	{
		if (m_form != kStrings || !m_fetchAll)
			throw Pire::Error("pire_hip: Rows() follows Run() and All()");
		FetchHits();
		return m_rows;
	}

private:
	SearchBatchRunner(const SearchBatchRunner&);
	SearchBatchRunner& operator=(const SearchBatchRunner&);

	enum Form { kNone, kStrings, kLines };
	SearchBatchRunner& SetBatch(Form form, const char* text, const uint64_t* offsets, size_t n, size_t len, char delim)
	{
		m_form = form, m_text = text, m_offsets = offsets, m_n = n, m_len = len, m_delim = uint8_t(delim);
		m_listed = m_haveText = false;
		return Select();
	}
	/* (the list form's entry points are named by All() alone: a program that never asks for it does not link them) */
	typedef void (SearchBatchRunner::*Fetch)();
	typedef int (*LinesCall)(pire_hip_table*, pire_hip_table*, uint32_t, const void*, uint64_t, uint32_t, uint32_t, uint32_t, uint64_t*, uint64_t*,
	                         uint64_t*, uint64_t, uint64_t*, void*, uint64_t, uint64_t*, uint64_t*, void*);
	SearchBatchRunner& SetAll(Fetch fetchAll, LinesCall linesCall)
	{
		if (m_fetchAll != fetchAll)
			m_listed = m_haveText = false;
		m_fetchAll = fetchAll, m_linesCall = linesCall;
		return *this;
	}
	void NeedLines(const char* what) const
	{
		if (m_form != kLines)
			throw Pire::Error(std::string("pire_hip: ") + what + " follows RunLines()");
	}

	/* All(): one call with room for a match per string -- RunLines(): per 64 bytes --, and a second one where there are more */
	void FetchAll()
	{
		const uint64_t* offsets = OwnedStrings::OffsetsOr(m_offsets, m_n);
		GrowAndRetry(m_form == kLines ? m_len / 64 + 1024 : m_n, [&](size_t cap) {
			m_hits.resize(cap);
			m_spans.resize(cap * 2);
			if (m_form == kStrings)
				m_rows.resize(m_n + 1);
			Check(m_form == kLines
			          ? m_linesCall(m_rev.Handle(), m_fwd.Handle(), m_opts, m_text, m_len, m_delim, 0, PIRE_HIP_GATHER_NO_TAIL, &m_lineCount,
			                        m_hits.data(), m_spans.data(), cap, &m_hitCount, nullptr, 0, nullptr, nullptr, nullptr)
			          : pire_hip_search_all(m_rev.Handle(), m_fwd.Handle(), m_opts, m_text, m_n ? offsets[m_n] : 0, offsets, m_n, 0, m_rows.data(),
			                                m_hits.data(), m_spans.data(), cap, &m_hitCount, nullptr));
			return size_t(m_hitCount);
		});
	}

	/* One call with room for every string -- RunLines(): for a hit on every line of 64 bytes or more, BatchRunner's first
	 * capacity --, and a second one where there are more */
	void FetchHits()
	{
		if (m_listed)
			return;
		if (m_form == kNone)
			throw Pire::Error("pire_hip: Hits() follows Run() or RunLines()");
		if (m_fetchAll) {
			(this->*m_fetchAll)();
			m_hits.resize(m_hitCount);
			m_spans.resize(m_hitCount * 2);
			m_listed = true;
			return;
		}
		GrowAndRetry(m_form == kLines ? m_len / 64 + 1024 : m_n, [&](size_t cap) {
			m_hits.resize(cap);
			m_spans.resize(cap * 2);
			Check(m_form == kLines
			          ? pire_hip_search_lines_gather(m_rev.Handle(), m_fwd.Handle(), m_opts, m_text, m_len, m_delim, 0, PIRE_HIP_GATHER_NO_TAIL,
			                                         &m_lineCount, m_hits.data(), m_spans.data(), cap, &m_hitCount, nullptr, 0, nullptr, nullptr,
			                                         nullptr)
			          : pire_hip_search_run_select(m_rev.Handle(), m_fwd.Handle(), m_opts, m_text, OwnedStrings::OffsetsOr(m_offsets, m_n), m_n, 0,
			                                       nullptr, nullptr, m_hits.data(), m_spans.data(), cap, &m_hitCount, nullptr));
			return size_t(m_hitCount);
		});
		m_hits.resize(m_hitCount);
		m_spans.resize(m_hitCount * 2);
		m_listed = true;
	}

	/* RunLines(): the matches as bytes; room for every byte they can have, and for the hits that are known, or else FetchHits()'s */
	void FetchHitText(char tail)
	{
		NeedLines("HitText()");
		if (m_haveText && m_textTail == tail)
			return;
		uint64_t count = 0, bytes = 0;
		GrowAndRetry(m_listed ? size_t(m_hitCount) : m_len / 64 + 1024, [&](size_t cap) {
			m_hitTextOffsets.resize(cap + 1);
			m_hitText.resize(m_len + cap + 1);
			Check(m_linesCall(m_rev.Handle(), m_fwd.Handle(), m_opts, m_text, m_len, m_delim, 0, uint8_t(tail), &m_lineCount, nullptr, nullptr, cap,
			                  &count, &m_hitText[0], m_hitText.size(), m_hitTextOffsets.data(), &bytes, nullptr));
			return size_t(count);   // (the text has room for the whole buffer and a tail per hit: where the hits fit, the bytes do)
		});
		m_hitText.resize(bytes);
		m_hitTextOffsets.resize(count + 1);
		m_textTail = tail;
		m_haveText = true;
	}

	Table<Scanner> m_rev, m_fwd;
	uint32_t m_opts;
	Form m_form;
	const char* m_text;           // Run(): the strings' text; RunLines(): the raw buffer of m_len bytes
	const uint64_t* m_offsets;
	size_t m_n, m_len;
	uint8_t m_delim;
	Fetch m_fetchAll;             // All(): every match, not the first of each string; null: the first
	LinesCall m_linesCall;        // the lines entry point of the selection
	bool m_listed, m_haveText;    // m_hits, m_spans (and m_lineCount) / m_hitText are the batch's, with the tail m_textTail
	char m_textTail;
	OwnedStrings m_ownStrings;
	uint64_t m_hitCount, m_lineCount;
	std::vector<uint64_t> m_hits, m_spans, m_rows, m_hitTextOffsets;
	std::string m_hitText;
};

/*
 * Both scanners of a search from ONE Pire::Fsm (not Surround()ed), and the runner over them:
 *     Pire::Hip::MatchFinder find(Pire::Lexer("[0-9]+").Parse());
 *     find.Runner().RunLines(raw, size).HitText();
 *   Forward()        the Fsm, compiled                                                     (pattern `re`)
 *   ReversedTail()   the Fsm + the lexer's `.*`, then Fsm::Reverse(), compiled             (pattern `(re).*`, reversed)
 * The tail is the LEXER's `.*` and not Fsm::AppendAnything(): that one loops on every letter, BeginMark and EndMark included
 * (fsm.cpp:1184-1196), and is another language wherever `re` takes a mark.
 */
class MatchFinder {
public:
	explicit MatchFinder(Pire::Fsm fsm, uint32_t opts = 0)
	    : m_fwd(Pire::Fsm(fsm).Compile<Pire::Scanner>()), m_rev(Tail(fsm).Reverse().Compile<Pire::Scanner>()), m_opts(opts), m_runner(m_rev, m_fwd, opts)
	{
	}
	const Pire::Scanner& Forward() const { return m_fwd; }
	const Pire::Scanner& ReversedTail() const { return m_rev; }
	uint32_t Opts() const { return m_opts; }
	SearchBatchRunner<Pire::Scanner>& Runner() { return m_runner; }

private:
	static Pire::Fsm Tail(const Pire::Fsm& fsm)
	{
		static const char kAny[] = ".*";
		return fsm + Pire::Lexer(kAny, kAny + 2).Parse();
	}
	Pire::Scanner m_fwd, m_rev;   // (declared before the runner that reads them)
	uint32_t m_opts;
	SearchBatchRunner<Pire::Scanner> m_runner;
};

/*
 * Which regexp each match belongs to, and tokens: pire_hip_lex / pire_hip_lex_lines_gather over a glued scanner (include/pire_hip.h,
 * "labelled matches and tokens").  The runner takes the two scanners of a TokenFinder (below) or the caller's own:
 *     Pire::Hip::LexBatchRunner lex(reversedTail, gluedForward);
 *     lex.Run(strings);                every leftmost-longest match of every string (SearchBatchRunner::All()'s) ...
 *     lex.Hits()  lex.Spans()  lex.Rows()  lex.HitCount()    ... as there, and per match:
 *     lex.Masks()        bit r: regexp r accepts the match                 lex.Labels()   its lowest regexp (lex's first-rule-wins)
 *     lex.LabelCounts()  [R + 1]: matches per label, gaps last -- counted on the device
 *     lex.Run(strings).Tokens();       maximal-munch tokens instead; what no regexp takes comes as gap entries, mask 0 and label
 *                                      kGap: the entries of a string tile it
 *     lex.RunLines(raw, size, '\n').Tokens().HitText('\n');   every token and gap of every line, a '\n' behind each
 * A new batch starts in search mode.  The caller's arrays are read when an accessor first asks: they live until then.
 */
class LexBatchRunner {
public:
	static const uint32_t kGap = 0xFFFFFFFFu;   // Labels(): the entry is a gap

	LexBatchRunner(const Pire::Scanner& reversedTail, const Pire::Scanner& forward, uint32_t opts = 0)
	    : m_rev(reversedTail), m_fwd(forward), m_regexps(forward.RegexpsCount()), m_opts(opts & ~uint32_t(PIRE_HIP_LEX_TOKENS)), m_mode(0),
	      m_form(kNone), m_text(nullptr), m_offsets(nullptr), m_n(0), m_len(0), m_delim('\n'), m_listed(false), m_haveText(false), m_textTail('\n'),
	      m_hitCount(0), m_lineCount(0)
	{
	}

	/* The batch: string i = text[offsets[i], offsets[i+1]).  Host pointers. */
	LexBatchRunner& Run(const char* text, const uint64_t* offsets, size_t n) { return SetBatch(kStrings, text, offsets, n, 0, '\n'); }
	LexBatchRunner& Run(const std::vector<ystring>& strings)
	{
		m_ownStrings.Assign(strings);
		return Run(m_ownStrings.Text(), m_ownStrings.Offsets(), strings.size());
	}
	LexBatchRunner& RunLines(const char* raw, size_t size, char delim = '\n') { return SetBatch(kLines, raw, nullptr, 0, size, delim); }
	/* tokens and gaps instead of matches (PIRE_HIP_LEX_TOKENS) */
	LexBatchRunner& Tokens(bool tokens = true)
	{
		const uint32_t mode = tokens ? PIRE_HIP_LEX_TOKENS : 0;
		if (mode != m_mode)
			m_listed = m_haveText = false;
		m_mode = mode;
		return *this;
	}
	uint64_t HitCount() { FetchHits("HitCount()"); return m_hitCount; }
	const std::vector<uint64_t>& Hits() { FetchHits("Hits()"); return m_hits; }
	const std::vector<uint64_t>& Spans() { FetchHits("Spans()"); return m_spans; }
	const std::vector<uint64_t>& Masks() { FetchHits("Masks()"); return m_masks; }
	const std::vector<uint32_t>& Labels() { FetchHits("Labels()"); return m_labels; }
	const std::vector<uint64_t>& LabelCounts() { FetchHits("LabelCounts()"); return m_labelCounts; }
	uint64_t LineCount() { NeedLines("LineCount()"); FetchHits("LineCount()"); return m_lineCount; }
	const std::string& HitText(char tail = '\n') { FetchHitText(tail); return m_hitText; }
	const std::vector<uint64_t>& HitTextOffsets()
	{
		if (!m_haveText)
			FetchHitText('\n');
		return m_hitTextOffsets;
	}
	/* behind Run(): n + 1 row starts into the lists */
	const std::vector<uint64_t>& Rows()
	{
		if (m_form != kStrings)
			throw Pire::Error("pire_hip: Rows() follows Run()");
		FetchHits("Rows()");
		return m_rows;
	}

private:
	LexBatchRunner(const LexBatchRunner&);
	LexBatchRunner& operator=(const LexBatchRunner&);

	enum Form { kNone, kStrings, kLines };
	LexBatchRunner& SetBatch(Form form, const char* text, const uint64_t* offsets, size_t n, size_t len, char delim)
	{
		m_form = form, m_text = text, m_offsets = offsets, m_n = n, m_len = len, m_delim = uint8_t(delim);
		m_listed = m_haveText = false;
		m_mode = 0;
		return *this;
	}
	void NeedLines(const char* what) const
	{
		if (m_form != kLines)
			throw Pire::Error(std::string("pire_hip: ") + what + " follows RunLines()");
	}

	/* One call with room for an entry per string -- RunLines(): per 64 bytes --, and a second one where there are more
	 * (SearchBatchRunner::FetchAll's capacities) */
	void FetchHits(const char* what)
	{
		if (m_listed)
			return;
		if (m_form == kNone)
			throw Pire::Error(std::string("pire_hip: ") + what + " follows Run() or RunLines()");
		const uint64_t* offsets = OwnedStrings::OffsetsOr(m_offsets, m_n);
		m_labelCounts.assign(size_t(m_regexps) + 1, 0);
		GrowAndRetry(m_form == kLines ? m_len / 64 + 1024 : m_n, [&](size_t cap) {
			m_hits.resize(cap);
			m_spans.resize(cap * 2);
			m_masks.resize(cap);
			if (m_form == kStrings)
				m_rows.resize(m_n + 1);
			Check(m_form == kLines
			          ? pire_hip_lex_lines_gather(m_rev.Handle(), m_fwd.Handle(), m_opts | m_mode, m_text, m_len, m_delim, 0, PIRE_HIP_GATHER_NO_TAIL,
			                                      &m_lineCount, m_hits.data(), m_spans.data(), m_masks.data(), cap, &m_hitCount, m_labelCounts.data(),
			                                      nullptr, 0, nullptr, nullptr, nullptr)
			          : pire_hip_lex(m_rev.Handle(), m_fwd.Handle(), m_opts | m_mode, m_text, m_n ? offsets[m_n] : 0, offsets, m_n, 0, m_rows.data(),
			                         m_hits.data(), m_spans.data(), m_masks.data(), cap, &m_hitCount, m_labelCounts.data(), nullptr));
			return size_t(m_hitCount);
		});
		m_hits.resize(m_hitCount);
		m_spans.resize(m_hitCount * 2);
		m_masks.resize(m_hitCount);
		m_labels.resize(m_hitCount);
		for (size_t k = 0; k < m_masks.size(); ++k) {
			uint32_t low = 0;
			while (low < 64 && !((m_masks[k] >> low) & 1))
				++low;
			m_labels[k] = low < 64 ? low : kGap;
		}
		m_listed = true;
	}

	/* RunLines(): the entries as bytes; room for every byte they can have, and for the entries that are known, or else FetchHits()'s */
	void FetchHitText(char tail)
	{
		NeedLines("HitText()");
		if (m_haveText && m_textTail == tail)
			return;
		uint64_t count = 0, bytes = 0;
		GrowAndRetry(m_listed ? size_t(m_hitCount) : m_len / 64 + 1024, [&](size_t cap) {
			m_hitTextOffsets.resize(cap + 1);
			m_hitText.resize(m_len + cap + 1);
			Check(pire_hip_lex_lines_gather(m_rev.Handle(), m_fwd.Handle(), m_opts | m_mode, m_text, m_len, m_delim, 0, uint8_t(tail), &m_lineCount,
			                                nullptr, nullptr, nullptr, cap, &count, nullptr, &m_hitText[0], m_hitText.size(), m_hitTextOffsets.data(),
			                                &bytes, nullptr));
			return size_t(count);   // (the text has room for the whole buffer and a tail per entry: where the entries fit, the bytes do)
		});
		m_hitText.resize(bytes);
		m_hitTextOffsets.resize(count + 1);
		m_textTail = tail;
		m_haveText = true;
	}

	Table<Pire::Scanner> m_rev, m_fwd;
	uint32_t m_regexps, m_opts, m_mode;   // m_mode: PIRE_HIP_LEX_TOKENS or 0
	Form m_form;
	const char* m_text;           // Run(): the strings' text; RunLines(): the raw buffer of m_len bytes
	const uint64_t* m_offsets;
	size_t m_n, m_len;
	uint8_t m_delim;
	bool m_listed, m_haveText;    // the lists (and m_lineCount) / m_hitText are the batch's in the present mode, with the tail m_textTail
	char m_textTail;
	OwnedStrings m_ownStrings;
	uint64_t m_hitCount, m_lineCount;
	std::vector<uint64_t> m_hits, m_spans, m_masks, m_labelCounts, m_rows, m_hitTextOffsets;
	std::vector<uint32_t> m_labels;
	std::string m_hitText;
};

/*
 * Both scanners of pire_hip_lex from the Fsms of the regexps (none Surround()ed), and the runner over them:
 *     std::vector<Pire::Fsm> rules;   rules.push_back(Pire::Lexer("[a-z]+").Parse());   rules.push_back(Pire::Lexer("[0-9]+").Parse());
 *     Pire::Hip::TokenFinder lexer(rules);
 *     lexer.Runner().RunLines(raw, size).Tokens().Labels();
 *   Forward()        Scanner::Glue of the compiled Fsms, in order: regexp r of the glued scanner is rules[r]
 *   ReversedTail()   the union of the Fsms + the lexer's `.*`, then Fsm::Reverse(), compiled   (MatchFinder's construction)
 * It throws Pire::Error for no Fsm, for more than 64, and where Glue answers the empty scanner (the product is too large).
 */
class TokenFinder {
public:
	explicit TokenFinder(const std::vector<Pire::Fsm>& fsms, uint32_t opts = 0)
	    : m_fwd(Glued(fsms)), m_rev(Tail(Union(fsms)).Reverse().Compile<Pire::Scanner>()), m_opts(opts), m_runner(m_rev, m_fwd, opts)
	{
	}
	const Pire::Scanner& Forward() const { return m_fwd; }
	const Pire::Scanner& ReversedTail() const { return m_rev; }
	uint32_t Opts() const { return m_opts; }
	LexBatchRunner& Runner() { return m_runner; }

private:
	static Pire::Scanner Glued(const std::vector<Pire::Fsm>& fsms)
	{
		if (fsms.empty() || fsms.size() > 64)
			throw Pire::Error("pire_hip: TokenFinder takes 1 to 64 regexps");
		Pire::Scanner glued = Pire::Fsm(fsms[0]).Compile<Pire::Scanner>();
		for (size_t i = 1; i < fsms.size(); ++i) {
			glued = Pire::Scanner::Glue(glued, Pire::Fsm(fsms[i]).Compile<Pire::Scanner>());
			if (glued.Empty())
				throw Pire::Error("pire_hip: TokenFinder: Scanner::Glue answered the empty scanner (the glued table is too large)");
		}
		return glued;
	}
	static Pire::Fsm Union(const std::vector<Pire::Fsm>& fsms)
	{
		Pire::Fsm all = fsms[0];
		for (size_t i = 1; i < fsms.size(); ++i)
			all |= fsms[i];
		return all;
	}
	static Pire::Fsm Tail(const Pire::Fsm& fsm)
	{
		static const char kAny[] = ".*";
		return fsm + Pire::Lexer(kAny, kAny + 2).Parse();
	}
	Pire::Scanner m_fwd, m_rev;   // (declared before the runner that reads them)
	uint32_t m_opts;
	LexBatchRunner m_runner;
};

/*
 * The matches of a buffer REPLACED, the rest kept -- `sed 's/re/repl/g'` on the device (pire_hip_search_lines_splice; the
 * delimiters are kept text, so Text() is the buffer as sed would print it and can go into the next RunLines()):
 *     Pire::Hip::MatchFinder find(Pire::Lexer("[0-9]+").Parse());
 *     Pire::Hip::Substitution sub(find);                    tables of its own over find's two scanners, find's opts
 *     sub.With("#").RunLines(raw, size, '\n');             every match becomes "#"
 *     sub.Text()  the rewritten buffer      sub.Bytes()  its size      sub.MatchCount()  matches replaced      sub.LineCount()
 *   With(repl)          the match is replaced by repl                              s/re/repl/g
 *   Wrap(head, tail)    the match stays, between head and tail                     s/re/head&tail/g, grep --color
 *   Delete()            the match goes                                             s/re//g            (what a new object does)
 *   FirstOnly(bool)     the first match of every line and not every match          s/re/repl/ ; an empty first match is an insertion
 * An empty match is never replaced without FirstOnly() (the list form of the search reports none).  head, tail and repl: at
 * most PIRE_HIP_SPLICE_PIECE_MAX bytes each.  The buffer is read when an accessor first asks: it lives until then.  One call at
 * a first capacity of matches and of bytes, and one more for each of the two that did not suffice (GrowAndRetry).
 */
class Substitution {
public:
	explicit Substitution(const MatchFinder& find)
	    : m_rev(find.ReversedTail()), m_fwd(find.Forward()), m_opts(find.Opts()), m_mode(0), m_raw(nullptr), m_len(0), m_delim('\n'), m_have(false),
	      m_done(false), m_matchCount(0), m_lineCount(0), m_bytes(0)
	{
	}
	Substitution& With(const std::string& repl) { return Piece(repl, std::string(), 0); }
	Substitution& Wrap(const std::string& head, const std::string& tail) { return Piece(head, tail, PIRE_HIP_SPLICE_KEEP); }
	Substitution& Delete() { return Piece(std::string(), std::string(), 0); }
	Substitution& FirstOnly(bool first = true)
	{
		m_mode = first ? m_mode | PIRE_HIP_SPLICE_FIRST : m_mode & ~uint32_t(PIRE_HIP_SPLICE_FIRST);
		m_done = false;
		return *this;
	}
	Substitution& RunLines(const char* raw, size_t size, char delim = '\n')
	{
		m_raw = raw, m_len = size, m_delim = uint8_t(delim);
		m_have = true, m_done = false;
		return *this;
	}
	const std::string& Text() { Fetch(); return m_text; }
	uint64_t Bytes() { Fetch(); return m_bytes; }
	uint64_t MatchCount() { Fetch(); return m_matchCount; }
	uint64_t LineCount() { Fetch(); return m_lineCount; }

private:
	Substitution(const Substitution&);
	Substitution& operator=(const Substitution&);

	Substitution& Piece(const std::string& head, const std::string& tail, uint32_t keep)
	{
		m_head = head, m_tail = tail;
		m_mode = (m_mode & PIRE_HIP_SPLICE_FIRST) | keep;
		m_done = false;
		return *this;
	}

	/* Room for a match per 64 bytes and for a result an eighth longer than the buffer; where the matches did not fit, that is
	 * settled first (the text of such a call is only partly rewritten), then the bytes. */
	void Fetch()
	{
		if (m_done)
			return;
		if (!m_have)
			throw Pire::Error("pire_hip: Text() follows RunLines()");
		size_t room = m_len + m_len / 8 + 64;
		GrowAndRetry(m_len / 64 + 1024, [&](size_t cap) {
			room = GrowAndRetry(room, [&](size_t textCap) {
				m_text.resize(textCap);
				Check(pire_hip_search_lines_splice(m_rev.Handle(), m_fwd.Handle(), m_opts, m_raw, m_len, m_delim, 0, m_head.data(), uint32_t(m_head.size()),
				                                   m_tail.data(), uint32_t(m_tail.size()), m_mode, &m_lineCount, nullptr, nullptr, cap, &m_matchCount,
				                                   &m_text[0], textCap, &m_bytes, nullptr));
				return m_matchCount <= cap ? size_t(m_bytes) : size_t(0);
			});
			return size_t(m_matchCount);
		});
		m_text.resize(m_bytes);
		m_done = true;
	}

	Table<Pire::Scanner> m_rev, m_fwd;
	uint32_t m_opts, m_mode;
	const char* m_raw;            // RunLines(): the raw buffer of m_len bytes
	size_t m_len;
	uint8_t m_delim;
	bool m_have, m_done;          // a buffer was given / m_text and the counts are its result under the present pieces
	std::string m_head, m_tail, m_text;
	uint64_t m_matchCount, m_lineCount, m_bytes;
};

}  // namespace Hip
}  // namespace Pire

#endif
