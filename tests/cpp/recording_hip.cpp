// A host-only stand-in for the part of the C ABI (include/pire_hip.h) that include/pire_hip/batch_runner.hpp calls.  Every
// function appends one line to a trace -- its name, every scalar argument, `null` or `set` for every pointer argument, and the
// contents of the small host arrays the header composes itself (offsets, text, want words, min thresholds) -- and answers what
// the driver scripted through the globals below.  No addresses, nothing that varies between runs.  "Device" memory is malloc,
// the copies are memcpy.  Linked into tests/cpp/shim_calls_test.cpp as an object file (tests/cpp/Makefile); it is never built
// as, or placed next to, libpire_hip.so.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <pire_hip.h>

// ---- what the driver sets ---------------------------------------------------------------------------------------------------
FILE* g_rec_out = nullptr;                  // the trace
uint32_t g_rec_regexps = 1;                 // pire_hip_table_info.regexps; mask words follow from it
uint64_t g_rec_hit_count = 0;               // what the next select / lines / count-select / capture calls report as hits
uint64_t g_rec_line_count = 0;              // ... as lines of the buffer
uint64_t g_rec_bytes = 0;                   // ... as gathered bytes
std::vector<uint64_t> g_rec_route_counts;   // ... per regexp, from route calls (missing entries are 0)
int g_rec_fail_next = 0;                    // the next call that can fail returns PIRE_HIP_EINVAL, once

// A line of the driver's own in the trace: the shaped results it saw
void rec_note(const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	fputs("# ", g_rec_out);
	vfprintf(g_rec_out, fmt, ap);
	fputc('\n', g_rec_out);
	va_end(ap);
}

namespace {

struct Handle {
	int id;
};
int g_handles = 0;

uint32_t MaskWords() { return g_rec_regexps ? (g_rec_regexps + 63) / 64 : 1; }

class Line {
public:
	explicit Line(const char* name) : m_text(name) {}
	~Line() { fprintf(g_rec_out, "%s\n", m_text.c_str()); }
	Line& Num(const char* key, uint64_t v) { return Add(key, std::to_string(v)); }
	Line& Int(const char* key, int64_t v) { return Add(key, std::to_string(v)); }
	Line& Ptr(const char* key, const void* p) { return Add(key, p ? "set" : "null"); }
	Line& Table(const char* key, const void* h) { return Add(key, h ? "#" + std::to_string(static_cast<const Handle*>(h)->id) : "null"); }
	template <class T>
	Line& Array(const char* key, const T* p, size_t n)
	{
		if (!p)
			return Add(key, "null");
		std::string s = "[";
		for (size_t i = 0; i < n; ++i)
			s += (i ? "," : "") + std::to_string(p[i]);
		return Add(key, s + "]");
	}
	Line& Bytes(const char* key, const void* p, size_t n)
	{
		if (!p)
			return Add(key, "null");
		if (n > 96)
			return Add(key, "set");
		std::string s = "\"";
		for (size_t i = 0; i < n; ++i) {
			const unsigned char c = static_cast<const unsigned char*>(p)[i];
			char hex[8];
			if (c >= 32 && c < 127 && c != '"' && c != '\\')
				s += char(c);
			else
				s += (snprintf(hex, sizeof(hex), "\\x%02x", c), hex);
		}
		return Add(key, s + "\"");
	}
	/* text and offsets of n strings: the offsets where they are few, and the bytes they span */
	Line& Strings(const void* text, const uint64_t* offsets, uint64_t n)
	{
		if (!offsets || n > 16)
			return Ptr("text", text).Ptr("offsets", offsets).Num("n", n);
		return Bytes("text", text, text ? size_t(offsets[n]) : 0).Array("offsets", offsets, size_t(n) + 1).Num("n", n);
	}
	Line& Raw(const void* raw, uint64_t size) { return Bytes("raw", raw, size_t(size)).Num("size", size); }
	Line& Want(const uint64_t* want) { return Array("want", want, MaskWords()); }
	Line& Min(const uint32_t* min) { return Array("min", min, g_rec_regexps); }

private:
	Line& Add(const char* key, const std::string& value)
	{
		m_text += std::string(" ") + key + "=" + value;
		return *this;
	}
	std::string m_text;
};

const char* g_error = "";

int Answer()
{
	if (g_rec_fail_next) {
		g_rec_fail_next = 0;
		g_error = "recording_hip: scripted refusal";
		return PIRE_HIP_EINVAL;
	}
	return PIRE_HIP_OK;
}

template <class T>
int Create(T** out)
{
	const int rc = Answer();
	if (rc == PIRE_HIP_OK) {
		Handle* h = new Handle;
		h->id = ++g_handles;
		*out = reinterpret_cast<T*>(h);
	}
	return rc;
}
template <class T>
void Destroy(T* t) { delete reinterpret_cast<Handle*>(t); }

template <class T>
void Fill(T* p, uint64_t n, T v)
{
	for (uint64_t i = 0; p && i < n; ++i)
		p[i] = v;
}
void Put(uint64_t* p, uint64_t v)
{
	if (p)
		*p = v;
}
void PutRouteCounts(uint64_t* counts)
{
	for (uint32_t r = 0; counts && r < g_rec_regexps; ++r)
		counts[r] = r < g_rec_route_counts.size() ? g_rec_route_counts[r] : 0;
}

}  // namespace

extern "C" {

uint32_t pire_hip_abi_version(void)
{
	Line("abi_version");
	return PIRE_HIP_ABI_VERSION;
}
const char* pire_hip_last_error(void)
{
	Line("last_error");
	return g_error;
}

int pire_hip_table_create(const void* blob, size_t len, pire_hip_table** out)
{
	const int rc = Create(out);
	Line("table_create").Ptr("blob", blob).Num("nonempty", len > 0).Table("out", rc ? nullptr : *out).Int("rc", rc);
	return rc;
}
void pire_hip_table_destroy(pire_hip_table* t)
{
	Line("table_destroy").Table("t", t);
	Destroy(t);
}
int pire_hip_counting_table_create(const void* blob, size_t len, pire_hip_counting_table** out)
{
	const int rc = Create(out);
	Line("counting_table_create").Ptr("blob", blob).Num("nonempty", len > 0).Table("out", rc ? nullptr : *out).Int("rc", rc);
	return rc;
}
void pire_hip_counting_table_destroy(pire_hip_counting_table* t)
{
	Line("counting_table_destroy").Table("t", t);
	Destroy(t);
}
int pire_hip_slow_table_create(const void* blob, size_t len, pire_hip_slow_table** out)
{
	const int rc = Create(out);
	Line("slow_table_create").Ptr("blob", blob).Num("nonempty", len > 0).Table("out", rc ? nullptr : *out).Int("rc", rc);
	return rc;
}
void pire_hip_slow_table_destroy(pire_hip_slow_table* t)
{
	Line("slow_table_destroy").Table("t", t);
	Destroy(t);
}
int pire_hip_table_get_info(const pire_hip_table* t, pire_hip_table_info* out)
{
	Line("table_get_info").Table("t", t).Ptr("out", out);
	memset(out, 0, sizeof(*out));
	out->abi_version = PIRE_HIP_ABI_VERSION;
	out->regexps = g_rec_regexps;
	return PIRE_HIP_OK;
}
uint32_t pire_hip_table_mask_words(const pire_hip_table* t)
{
	Line("table_mask_words").Table("t", t);
	return MaskWords();
}
int pire_hip_table_adapt(pire_hip_table* t, uint32_t* changed)
{
	Line("table_adapt").Table("t", t).Ptr("changed", changed);
	*changed = 3;
	return Answer();
}
int pire_hip_config_get(pire_hip_config* out)
{
	Line("config_get").Num("size_ok", out->size == sizeof(*out));
	const uint32_t size = out->size;
	memset(out, 0, sizeof(*out));
	out->size = size;
	return Answer();
}
int pire_hip_config_set(const pire_hip_config* in)
{
	Line("config_set").Num("size_ok", in->size == sizeof(*in)).Num("auto_adapt", in->auto_adapt);
	return Answer();
}

int pire_hip_device_alloc(size_t bytes, void** out)
{
	Line("device_alloc").Num("bytes", bytes);
	*out = calloc(bytes ? bytes : 1, 1);
	return Answer();
}
void pire_hip_device_free(void* p)
{
	Line("device_free").Ptr("p", p);
	free(p);
}
int pire_hip_copy_to_host(void* dst, const void* src, size_t bytes, void* stream)
{
	Line("copy_to_host").Ptr("dst", dst).Ptr("src", src).Num("bytes", bytes).Ptr("stream", stream);
	if (bytes)
		memcpy(dst, src, bytes);
	return Answer();
}
int pire_hip_copy_to_device(void* dst, const void* src, size_t bytes, void* stream)
{
	// (the header's own sources: From()'s state indices, Select()'s want words)
	Line("copy_to_device").Ptr("dst", dst).Array("src", static_cast<const uint32_t*>(src), bytes <= 64 ? bytes / 4 : 0).Num("bytes", bytes)
	    .Ptr("stream", stream);
	if (bytes)
		memcpy(dst, src, bytes);
	return Answer();
}
int pire_hip_memset_device(void* dst, int value, size_t bytes, void* stream)
{
	Line("memset_device").Ptr("dst", dst).Int("value", value).Num("bytes", bytes).Ptr("stream", stream);
	if (bytes)
		memset(dst, value, bytes);
	return Answer();
}
int pire_hip_stream_synchronize(void* stream)
{
	Line("stream_synchronize").Ptr("stream", stream);
	return Answer();
}

int pire_hip_run(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags, const uint32_t* init,
                 uint32_t* out_idx, uint8_t* out_final, uint64_t* out_counts, void* stream)
{
	Line("run").Table("t", t).Strings(text, offsets, n).Num("flags", flags).Array("init", init, n <= 16 ? size_t(n) : 0).Ptr("out_idx", out_idx)
	    .Ptr("out_final", out_final).Ptr("out_counts", out_counts).Ptr("stream", stream);
	const int rc = Answer();
	if (rc == PIRE_HIP_OK) {
		Fill(out_idx, n, uint32_t(0));
		Fill(out_final, n, uint8_t(1));
		Put(out_counts, n);
	}
	return rc;
}
int pire_hip_run_strided(pire_hip_table* t, const void* text, uint64_t n, uint64_t len, uint64_t stride, uint32_t flags, const uint32_t* init,
                         uint32_t* out_idx, uint8_t* out_final, uint64_t* out_counts, void* stream)
{
	Line("run_strided").Table("t", t).Ptr("text", text).Num("n", n).Num("len", len).Num("stride", stride).Num("flags", flags)
	    .Array("init", init, n <= 16 ? size_t(n) : 0).Ptr("out_idx", out_idx).Ptr("out_final", out_final).Ptr("out_counts", out_counts)
	    .Ptr("stream", stream);
	Fill(out_idx, n, uint32_t(0));
	Fill(out_final, n, uint8_t(1));
	Put(out_counts, n);
	return Answer();
}
int pire_hip_run_pair_strided(pire_hip_table* t1, pire_hip_table* t2, const void* text, uint64_t n, uint64_t len, uint64_t stride, uint32_t flags,
                              uint32_t* out_idx1, uint32_t* out_idx2, uint8_t* out_final, void* stream)
{
	Line("run_pair_strided").Table("t1", t1).Table("t2", t2).Ptr("text", text).Num("n", n).Num("len", len).Num("stride", stride)
	    .Num("flags", flags).Ptr("out_idx1", out_idx1).Ptr("out_idx2", out_idx2).Ptr("out_final", out_final).Ptr("stream", stream);
	Fill(out_idx1, n, uint32_t(0));
	Fill(out_idx2, n, uint32_t(0));
	Fill(out_final, n, uint8_t(1));
	return Answer();
}
int pire_hip_select(pire_hip_table* t, const uint32_t* state_idx, uint64_t n, const uint64_t* want, uint32_t flags, uint64_t* out_masks,
                    uint64_t* out_hits, uint64_t* out_hit_masks, uint64_t hit_cap, uint64_t* out_hit_count, void* stream)
{
	Line("select").Table("t", t).Ptr("state_idx", state_idx).Num("n", n).Want(want).Num("flags", flags).Ptr("out_masks", out_masks)
	    .Ptr("out_hits", out_hits).Ptr("out_hit_masks", out_hit_masks).Num("hit_cap", hit_cap).Ptr("out_hit_count", out_hit_count)
	    .Ptr("stream", stream);
	Put(out_hit_count, g_rec_hit_count < n ? g_rec_hit_count : n);
	return Answer();
}
int pire_hip_route(pire_hip_table* t, const uint32_t* state_idx, uint64_t n, uint32_t flags, uint64_t* out_hits, uint64_t hit_cap,
                   uint64_t* out_hit_counts, void* stream)
{
	Line("route").Table("t", t).Ptr("state_idx", state_idx).Num("n", n).Num("flags", flags).Ptr("out_hits", out_hits).Num("hit_cap", hit_cap)
	    .Ptr("out_hit_counts", out_hit_counts).Ptr("stream", stream);
	PutRouteCounts(out_hit_counts);
	return Answer();
}

int pire_hip_run_lines_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, const uint64_t* want,
                              uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans, uint64_t* out_hit_masks, uint64_t hit_cap,
                              uint64_t* out_hit_count, void* stream)
{
	Line("run_lines_select").Table("t", t).Raw(raw, size).Num("delim", delim).Num("flags", flags).Want(want).Ptr("out_line_count", out_line_count)
	    .Ptr("out_hits", out_hits).Ptr("out_hit_spans", out_hit_spans).Ptr("out_hit_masks", out_hit_masks).Num("hit_cap", hit_cap)
	    .Ptr("out_hit_count", out_hit_count).Ptr("stream", stream);
	Put(out_line_count, g_rec_line_count);
	Put(out_hit_count, g_rec_hit_count);
	return Answer();
}
int pire_hip_run_lines_field_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t sep, uint32_t field, uint32_t mode,
                                    uint32_t flags, const uint64_t* want, uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans,
                                    uint64_t* out_hit_masks, uint64_t hit_cap, uint64_t* out_hit_count, void* stream)
{
	Line("run_lines_field_select").Table("t", t).Raw(raw, size).Num("delim", delim).Num("sep", sep).Num("field", field).Num("mode", mode)
	    .Num("flags", flags).Want(want).Ptr("out_line_count", out_line_count).Ptr("out_hits", out_hits).Ptr("out_hit_spans", out_hit_spans)
	    .Ptr("out_hit_masks", out_hit_masks).Num("hit_cap", hit_cap).Ptr("out_hit_count", out_hit_count).Ptr("stream", stream);
	Put(out_line_count, g_rec_line_count);
	Put(out_hit_count, g_rec_hit_count);
	return Answer();
}
int pire_hip_run_lines_gather(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, const uint64_t* want, uint32_t tail,
                              uint64_t* out_line_count, uint64_t* out_hits, uint64_t hit_cap, uint64_t* out_hit_count, void* out_text,
                              uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* stream)
{
	Line("run_lines_gather").Table("t", t).Raw(raw, size).Num("delim", delim).Num("flags", flags).Want(want).Num("tail", tail)
	    .Ptr("out_line_count", out_line_count).Ptr("out_hits", out_hits).Num("hit_cap", hit_cap).Ptr("out_hit_count", out_hit_count)
	    .Ptr("out_text", out_text).Num("text_cap", text_cap).Ptr("out_offsets", out_offsets).Ptr("out_bytes", out_bytes).Ptr("stream", stream);
	Put(out_line_count, g_rec_line_count);
	Put(out_hit_count, g_rec_hit_count);
	Put(out_bytes, g_rec_bytes);
	return Answer();
}
int pire_hip_run_lines_field_gather(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t sep, uint32_t field, uint32_t mode,
                                    uint32_t flags, const uint64_t* want, uint32_t tail, uint64_t* out_line_count, uint64_t* out_hits,
                                    uint64_t hit_cap, uint64_t* out_hit_count, void* out_text, uint64_t text_cap, uint64_t* out_offsets,
                                    uint64_t* out_bytes, void* stream)
{
	Line("run_lines_field_gather").Table("t", t).Raw(raw, size).Num("delim", delim).Num("sep", sep).Num("field", field).Num("mode", mode)
	    .Num("flags", flags).Want(want).Num("tail", tail).Ptr("out_line_count", out_line_count).Ptr("out_hits", out_hits).Num("hit_cap", hit_cap)
	    .Ptr("out_hit_count", out_hit_count).Ptr("out_text", out_text).Num("text_cap", text_cap).Ptr("out_offsets", out_offsets)
	    .Ptr("out_bytes", out_bytes).Ptr("stream", stream);
	Put(out_line_count, g_rec_line_count);
	Put(out_hit_count, g_rec_hit_count);
	Put(out_bytes, g_rec_bytes);
	return Answer();
}
int pire_hip_run_lines_route(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint64_t* out_line_count,
                             uint64_t* out_hits, uint64_t* out_hit_spans, uint64_t hit_cap, uint64_t* out_hit_counts, void* stream)
{
	Line("run_lines_route").Table("t", t).Raw(raw, size).Num("delim", delim).Num("flags", flags).Ptr("out_line_count", out_line_count)
	    .Ptr("out_hits", out_hits).Ptr("out_hit_spans", out_hit_spans).Num("hit_cap", hit_cap).Ptr("out_hit_counts", out_hit_counts)
	    .Ptr("stream", stream);
	Put(out_line_count, g_rec_line_count);
	PutRouteCounts(out_hit_counts);
	return Answer();
}

int pire_hip_prefix(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, int longest, int through_begin, int through_end,
                    uint32_t flags, int64_t* out_len, void* stream)
{
	Line("prefix").Table("t", t).Strings(text, offsets, n).Int("longest", longest).Int("through_begin", through_begin)
	    .Int("through_end", through_end).Num("flags", flags).Ptr("out_len", out_len).Ptr("stream", stream);
	for (uint64_t i = 0; i < n; ++i)
		out_len[i] = i % 2 ? -1 : 1;
	return Answer();
}
int pire_hip_suffix(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, int longest, int through_end, int through_begin,
                    uint32_t flags, int64_t* out_len, void* stream)
{
	Line("suffix").Table("t", t).Strings(text, offsets, n).Int("longest", longest).Int("through_end", through_end)
	    .Int("through_begin", through_begin).Num("flags", flags).Ptr("out_len", out_len).Ptr("stream", stream);
	for (uint64_t i = 0; i < n; ++i)
		out_len[i] = i % 2 ? -1 : 1;
	return Answer();
}

int pire_hip_multi_create(const int* devices, int ndev, pire_hip_multi** out)
{
	const int rc = Create(out);
	Line("multi_create").Array("devices", devices, size_t(ndev)).Int("ndev", ndev).Table("out", rc ? nullptr : *out).Int("rc", rc);
	return rc;
}
void pire_hip_multi_destroy(pire_hip_multi* m)
{
	Line("multi_destroy").Table("m", m);
	Destroy(m);
}
int pire_hip_multi_device_count(const pire_hip_multi* m)
{
	Line("multi_device_count").Table("m", m);
	return 2;
}
const char* pire_hip_multi_reduce_backend(const pire_hip_multi* m)
{
	Line("multi_reduce_backend").Table("m", m);
	return "host";
}
int pire_hip_multi_run_host(pire_hip_multi* m, pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                            const uint32_t* init, uint32_t* out_idx, uint8_t* out_final, uint64_t* out_counts)
{
	Line("multi_run_host").Table("m", m).Table("t", t).Strings(text, offsets, n).Num("flags", flags).Ptr("init", init).Ptr("out_idx", out_idx)
	    .Ptr("out_final", out_final).Ptr("out_counts", out_counts);
	Fill(out_idx, n, uint32_t(0));
	Fill(out_final, n, uint8_t(1));
	Put(out_counts, n);
	return Answer();
}

int pire_hip_run_half_final(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags, uint32_t* out_idx,
                            uint8_t* out_final, uint32_t* out_results, void* stream)
{
	Line("run_half_final").Table("t", t).Strings(text, offsets, n).Num("flags", flags).Ptr("out_idx", out_idx).Ptr("out_final", out_final)
	    .Ptr("out_results", out_results).Ptr("stream", stream);
	Fill(out_final, n, uint8_t(1));
	Fill(out_results, n * g_rec_regexps, uint32_t(7));
	return Answer();
}
int pire_hip_run_half_final_select(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags, uint32_t* out_idx,
                                   uint8_t* out_final, uint32_t* out_results, const uint32_t* min, uint32_t mode, uint64_t* out_totals,
                                   uint64_t* out_hits, uint32_t* out_hit_results, uint64_t hit_cap, uint64_t* out_hit_count, void* stream)
{
	Line("run_half_final_select").Table("t", t).Strings(text, offsets, n).Num("flags", flags).Ptr("out_idx", out_idx).Ptr("out_final", out_final)
	    .Ptr("out_results", out_results).Min(min).Num("mode", mode).Ptr("out_totals", out_totals).Ptr("out_hits", out_hits)
	    .Ptr("out_hit_results", out_hit_results).Num("hit_cap", hit_cap).Ptr("out_hit_count", out_hit_count).Ptr("stream", stream);
	const int rc = Answer();
	if (rc == PIRE_HIP_OK)
		Put(out_hit_count, g_rec_hit_count);
	return rc;
}
int pire_hip_half_final_lines_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, const uint32_t* min,
                                     uint32_t mode, uint64_t* out_line_count, uint64_t* out_totals, uint64_t* out_hits, uint64_t* out_hit_spans,
                                     uint32_t* out_hit_results, uint64_t hit_cap, uint64_t* out_hit_count, void* stream)
{
	Line("half_final_lines_select").Table("t", t).Raw(raw, size).Num("delim", delim).Num("flags", flags).Min(min).Num("mode", mode)
	    .Ptr("out_line_count", out_line_count).Ptr("out_totals", out_totals).Ptr("out_hits", out_hits).Ptr("out_hit_spans", out_hit_spans)
	    .Ptr("out_hit_results", out_hit_results).Num("hit_cap", hit_cap).Ptr("out_hit_count", out_hit_count).Ptr("stream", stream);
	Put(out_line_count, g_rec_line_count);
	Put(out_hit_count, g_rec_hit_count);
	return Answer();
}
int pire_hip_counting_run(pire_hip_counting_table* t, int kind, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                          uint32_t* out_idx, uint32_t* out_results, void* stream)
{
	Line("counting_run").Table("t", t).Int("kind", kind).Strings(text, offsets, n).Num("flags", flags).Ptr("out_idx", out_idx)
	    .Ptr("out_results", out_results).Ptr("stream", stream);
	Fill(out_results, n * g_rec_regexps, uint32_t(7));
	return Answer();
}
int pire_hip_counting_run_select(pire_hip_counting_table* t, int kind, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                                 uint32_t* out_idx, uint32_t* out_results, const uint32_t* min, uint32_t mode, uint64_t* out_totals,
                                 uint64_t* out_hits, uint32_t* out_hit_results, uint64_t hit_cap, uint64_t* out_hit_count, void* stream)
{
	Line("counting_run_select").Table("t", t).Int("kind", kind).Strings(text, offsets, n).Num("flags", flags).Ptr("out_idx", out_idx)
	    .Ptr("out_results", out_results).Min(min).Num("mode", mode).Ptr("out_totals", out_totals).Ptr("out_hits", out_hits)
	    .Ptr("out_hit_results", out_hit_results).Num("hit_cap", hit_cap).Ptr("out_hit_count", out_hit_count).Ptr("stream", stream);
	const int rc = Answer();
	if (rc == PIRE_HIP_OK)
		Put(out_hit_count, g_rec_hit_count);
	return rc;
}
int pire_hip_counting_lines_select(pire_hip_counting_table* t, int kind, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                   const uint32_t* min, uint32_t mode, uint64_t* out_line_count, uint64_t* out_totals, uint64_t* out_hits,
                                   uint64_t* out_hit_spans, uint32_t* out_hit_results, uint64_t hit_cap, uint64_t* out_hit_count, void* stream)
{
	Line("counting_lines_select").Table("t", t).Int("kind", kind).Raw(raw, size).Num("delim", delim).Num("flags", flags).Min(min).Num("mode", mode)
	    .Ptr("out_line_count", out_line_count).Ptr("out_totals", out_totals).Ptr("out_hits", out_hits).Ptr("out_hit_spans", out_hit_spans)
	    .Ptr("out_hit_results", out_hit_results).Num("hit_cap", hit_cap).Ptr("out_hit_count", out_hit_count).Ptr("stream", stream);
	Put(out_line_count, g_rec_line_count);
	Put(out_hit_count, g_rec_hit_count);
	return Answer();
}

int pire_hip_capture_run(pire_hip_counting_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags, uint32_t* out_idx,
                         uint8_t* out_final, int64_t* out_begin, int64_t* out_end, void* stream)
{
	Line("capture_run").Table("t", t).Strings(text, offsets, n).Num("flags", flags).Ptr("out_idx", out_idx).Ptr("out_final", out_final)
	    .Ptr("out_begin", out_begin).Ptr("out_end", out_end).Ptr("stream", stream);
	Fill(out_begin, n, int64_t(2));
	Fill(out_end, n, int64_t(3));
	return Answer();
}
int pire_hip_capture_run_select(pire_hip_counting_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags, int need_final,
                                uint32_t* out_idx, uint8_t* out_final, int64_t* out_begin, int64_t* out_end, uint64_t* out_hits,
                                uint64_t* out_spans, uint64_t hit_cap, uint64_t* out_hit_count, void* stream)
{
	Line("capture_run_select").Table("t", t).Strings(text, offsets, n).Num("flags", flags).Int("need_final", need_final).Ptr("out_idx", out_idx)
	    .Ptr("out_final", out_final).Ptr("out_begin", out_begin).Ptr("out_end", out_end).Ptr("out_hits", out_hits).Ptr("out_spans", out_spans)
	    .Num("hit_cap", hit_cap).Ptr("out_hit_count", out_hit_count).Ptr("stream", stream);
	Fill(out_begin, n, int64_t(2));
	Fill(out_end, n, int64_t(3));
	Put(out_hit_count, g_rec_hit_count < n ? g_rec_hit_count : n);
	return Answer();
}
int pire_hip_capture_lines_gather(pire_hip_counting_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags, int need_final,
                                  uint32_t tail, uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap,
                                  uint64_t* out_hit_count, void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes,
                                  void* stream)
{
	Line("capture_lines_gather").Table("t", t).Raw(raw, size).Num("delim", delim).Num("flags", flags).Int("need_final", need_final)
	    .Num("tail", tail).Ptr("out_line_count", out_line_count).Ptr("out_hits", out_hits).Ptr("out_spans", out_spans).Num("hit_cap", hit_cap)
	    .Ptr("out_hit_count", out_hit_count).Ptr("out_text", out_text).Num("text_cap", text_cap).Ptr("out_offsets", out_offsets)
	    .Ptr("out_bytes", out_bytes).Ptr("stream", stream);
	Put(out_line_count, g_rec_line_count);
	Put(out_hit_count, g_rec_hit_count);
	Put(out_bytes, g_rec_bytes);
	return Answer();
}

int pire_hip_slow_run(pire_hip_slow_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags, uint8_t* out_final,
                      uint32_t* out_state_bits, uint64_t* out_counts, void* stream)
{
	Line("slow_run").Table("t", t).Strings(text, offsets, n).Num("flags", flags).Ptr("out_final", out_final).Ptr("out_state_bits", out_state_bits)
	    .Ptr("out_counts", out_counts).Ptr("stream", stream);
	Fill(out_final, n, uint8_t(1));
	return Answer();
}

}  // extern "C"
