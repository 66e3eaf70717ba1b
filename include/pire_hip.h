/*
 * pire_hip.h -- C ABI of libpire_hip.so: the MI355X (gfx950) implementation of Pire's scan path.
 *
 * Scope: exactly one reference path --
 *     Pire::Runner(scanner).Begin().Run(ptr, len).End()            (pire/run.h:365-392)
 * i.e. the DFA walk  Step(BeginMark); Run(begin,end); Step(EndMark)  (run.h:50-57, 271-275) over a
 * compiled Pire::Scanner / Pire::NonrelocScanner table (pire/scanners/multi.h:87-554), batched over
 * N independent strings, one string per GPU lane.  Regex parsing, FSM construction, determinisation,
 * minimisation and Scanner::Glue stay in the reference library on the host; the hand-off between the
 * two is the reference's PUBLIC serialised form, Scanner::Save() (multi.h:557-573, 620-624).
 *
 * The reference has no FFI for this path: it is a header-only C++ template concept.  The binding a
 * Pire maintainer would add is therefore a C++ shim over this C ABI (include/pire_hip/batch_runner.hpp,
 * INTEGRATION.md).  All entry points take plain pointers and sizes; no C++ / torch types.
 *
 * Results are bit-exact with the reference: for every string, the StateIndex (multi.h:281-284) of the
 * state the reference would end in, and its Final flag (multi.h:143).
 *
 * Error model (the reference throws Pire::Error, pire/stub/stl.h:213-217): every call returns
 * PIRE_HIP_OK (0) or a negative code; pire_hip_last_error() returns the thread-local message.
 * There is NO CPU fallback: without a usable HIP device every run call fails with PIRE_HIP_ENODEVICE.
 */
#ifndef PIRE_HIP_H
#define PIRE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIRE_HIP_ABI_VERSION 6

enum {
	PIRE_HIP_OK        =  0,
	PIRE_HIP_EINVAL    = -1,   /* bad argument                                                        */
	PIRE_HIP_EFORMAT   = -2,   /* blob rejected: same checks as Header::Validate, common.h:65-77,     */
	                           /* and Scanner::Load, multi.h:575-599                                  */
	PIRE_HIP_ENODEVICE = -3,   /* no HIP device / HIP runtime error (message has the hipError string) */
	PIRE_HIP_ENOMEM    = -4,
	PIRE_HIP_EUNSUPPORTED = -5,
	PIRE_HIP_ESELFTEST = -6    /* a kernel's first-use known-answer batch came back wrong (pire_hip_config.selftest):   */
	                           /* this build of the library must not be used on this device; no results were written   */
};

/* run flags */
enum {
	PIRE_HIP_RUN_BEGIN     = 1u << 0,   /* Step(BeginMark) before the text  -- RunHelper::Begin(), run.h:375 */
	PIRE_HIP_RUN_END       = 1u << 1,   /* Step(EndMark) after the text     -- RunHelper::End(),   run.h:376 */
	PIRE_HIP_RUN_ON_DEVICE = 1u << 2,   /* text/offsets/init/out pointers are DEVICE pointers; the call only */
	                                    /* enqueues work on `stream`. Without it they are HOST pointers and  */
	                                    /* the call copies in, runs, copies out and synchronises.            */
	                                    /* What can still make an ON_DEVICE call wait, and how to switch it   */
	                                    /* off (pire_hip_config): (1) pire_hip_run with DEVICE offsets and    */
	                                    /* n < 65 536 reads the first and last offset back (synchronises      */
	                                    /* `stream`) to spot few long strings -- no_offsets_peek = 1; (2) a   */
	                                    /* call that ends up in the segmented scan (few long strings of known */
	                                    /* length: strided records, HOST_OFFSETS, or the peek) synchronises   */
	                                    /* `stream` while it follows the chain -- no_segments = 1; (3) the    */
	                                    /* first call on a device uploads the table (hipMalloc + copies):     */
	                                    /* pire_hip_table_upload() beforehand.  With those three an ON_DEVICE */
	                                    /* call enqueues kernels and nothing else (it is then legal inside a  */
	                                    /* stream capture).  Automatic adaptation (auto_adapt) never runs     */
	                                    /* inside an ON_DEVICE call unless auto_adapt = 2.                    */
	                                    /* A graph captured from ON_DEVICE calls holds the pointers of the    */
	                                    /* table's device image: an AUTOMATIC adaptation keeps the images it  */
	                                    /* replaces alive until pire_hip_table_destroy() (a replay walks the  */
	                                    /* old ranking: same results); after the caller's OWN                 */
	                                    /* pire_hip_table_adapt() the old images are freed -- re-capture.     */
	                                    /* Device text is read in whole 128-byte aligned lines: the kernels   */
	                                    /* may load (never use) up to 127 bytes in front of the first and     */
	                                    /* behind the last byte of the text -- always inside the memory page  */
	                                    /* that holds that byte, so any device allocation will do.            */
	PIRE_HIP_RUN_GENERIC   = 1u << 3,   /* force the generic (offset-driven) kernel; testing/diagnostics     */
	PIRE_HIP_RUN_NO_PEEK   = 1u << 5,   /* with ON_DEVICE, pire_hip_run: this call never reads device offsets  */
	                                    /* back (what pire_hip_config.no_offsets_peek is for every call)       */
	PIRE_HIP_RUN_HOST_OFFSETS = 1u << 4 /* with ON_DEVICE, pire_hip_run only: `offsets` is a HOST pointer (the  */
	                                    /* text stays resident on the device, the caller knows where its        */
	                                    /* documents start).  The call copies the offsets and synchronises      */
	                                    /* `stream` before it returns; because the host then knows the lengths, */
	                                    /* few long strings get the segmented scan described at pire_hip_run.   */
};

typedef struct pire_hip_table pire_hip_table;

/* ---- library configuration ------------------------------------------------------------------------
 * The runtime knobs of the library, set through the ABI.  Process-wide; a call takes a snapshot
 * when it starts, so pire_hip_config_set() affects the calls that start after it.  0 = the default everywhere.
 * The environment variables of the same names in upper case with the prefix PIRE_HIP_ (PIRE_HIP_TILED_VARIANT,
 * PIRE_HIP_NO_SEGMENTS, ...) are read ONCE, when the library is loaded, and only seed this struct: no launch path
 * calls getenv().  `size` = sizeof(pire_hip_config) of the caller: the struct may grow at its end. */
typedef struct pire_hip_config {
	uint32_t size;
	/* fixed-length records (pire_hip_run_strided) */
	uint32_t tiled_variant;        /* 0 the shipped kernel; 23 dense rows with rotated columns (LDS bank = byte & 63; no  */
	                               /* gain measured, round 4); 2 without `nt`; 20 waves not kept in step; 22 the transpose */
	                               /* of the next tile hidden in the walk; 1 rows 260 bytes apart: A/B measurements, same  */
	                               /* results                                                                               */
	uint32_t checked;              /* 1: the checked kernel build, see pire_hip_table_check_failures()                 */
	/* tables (applies to tables created / glued afterwards) */
	uint32_t no_compact;           /* 1: no compact LDS tier behind the dense rows                                      */
	uint32_t prior_flat;           /* 1: an a-priori ranking that knows nothing (tests of adapt())                      */
	/* offset batches with actions (prefix searches, HalfFinal counting) */
	uint32_t ragged_act_always;    /* 1: never take the one-string-per-lane kernel for "quick" searches                 */
	uint32_t no_ragged_act;        /* 1: always take it                                                                 */
	/* few long strings: the segmented scan */
	uint32_t no_segments;          /* 1: never                                                                          */
	uint32_t segment_no_grid;      /* 1: every segment through the ragged kernel                                        */
	uint32_t segment_stats;        /* 1: print a host timeline per call (synchronises at every mark)                    */
	uint32_t segment_modes;        /* modes per call (default 6)                                                        */
	uint64_t segment_bytes;        /* bytes per segment; non-zero also FORCES the segmented scan for every eligible call */
	uint64_t segment_warmup;       /* warm-up bytes in front of a segment (default 256); SEGMENT_WARMUP_NONE = 0 bytes   */
	uint64_t segment_budget;       /* chain repair rounds (default 32); SEGMENT_BUDGET_NONE = 0 rounds                   */
	/* host-pointer mode */
	uint64_t host_chunk_bytes;     /* staging chunk size (default 256 MiB, minimum 4096)                                */
	uint32_t host_one_shot;        /* 1: one allocation + one copy per call instead of the pooled pipeline              */
	/* multi-device */
	uint32_t no_rccl;              /* 1: sum the per-device counters on the host                                        */
	/* SlowScanner */
	uint32_t slow_sets_in_memory;  /* 1: the wave-per-string form keeps its state sets in device memory                 */
	uint32_t slow_no_list;         /* 1: never the 16-slot list kernel: bitset kernel (<= 256 states) / wave per string   */
	/* adaptation of the dense-row ranking */
	uint32_t auto_adapt;           /* re-rank the LDS rows by itself when scans keep leaving them (see                   */
	                               /* pire_hip_table_adapt()): 0 default = in calls that synchronise anyway (host-pointer */
	                               /* forms, HOST_OFFSETS) right there -- the device is drained (hipDeviceSynchronize) --, */
	                               /* and in calls that only enqueue (ON_DEVICE) IN THE BACKGROUND: a worker thread copies */
	                               /* the counters on a stream of its own, re-ranks a copy of the table, uploads the new   */
	                               /* image, and a later launch boundary swaps it in -- such a call never waits for the    */
	                               /* device and stays legal inside a stream capture; 1 never; 2 at every launch boundary, */
	                               /* draining the device, ON_DEVICE calls included (such a call may then block and is not */
	                               /* capturable); 3 round 5's default: never inside a call that only enqueues             */
	uint32_t auto_adapt_min_traps; /* sampled trap count since the last ranking that triggers it (default 256)          */
	/* offset batches (pire_hip_run) */
	uint32_t ragged_variant;       /* 0 default: large offset batches (>= 160 MiB of text when the host knows the lengths, */
	                               /* >= 2^20 strings when the offsets are on the device) take the stream kernel (every    */
	                               /* lane walks a run of consecutive strings), smaller ones the ragged kernel (one string */
	                               /* per lane at a time); 1 always the ragged kernel; 2 the stream kernel from 256        */
	                               /* strings (tests) -- and, for tables on the class-indexed walk, the stream kernel on   */
	                               /* that walk, which 0 never takes (measured slower there; its image is  */
	                               /* built for tables uploaded while 2 is set).  Same results either way.                 */
	uint32_t host_staging;         /* device staging of the host-pointer forms of the prefix / suffix / half-final /   */
	                               /* counting / capture / slow entry points: 0 blocks cached per device between calls */
	                               /* (no allocation in steady state), 1 hipMalloc + hipFree per call (round 2),       */
	                               /* 2 the stream-ordered pool (hipMallocAsync): measurements                          */
	uint32_t no_offsets_peek;      /* 1: pire_hip_run with device offsets never reads offsets back (enqueue-only even for */
	                               /* small batches; few long strings then walk one per lane)                            */
	uint32_t segment_no_pair;      /* 1: the segmented scan never fuses two modes into one pass of the pair kernel       */
	uint32_t segment_no_product;   /* 1: two modes that are not functions of each other take the pair kernel, not a product */
	uint32_t segment_no_derive;    /* 1: the segmented scan walks every mode (none derived from mode 0's walk)           */
	uint32_t no_length_order;      /* 1: counting / SlowScanner kernels take strings in the caller's order, not by length */
	uint32_t capture_by_length;    /* 1: the one-string-per-lane capture kernels too take them by length (A/B: slower)   */
	uint32_t force_rccl;           /* 1: pire_hip_multi_create builds an RCCL communicator for ONE device as well (a       */
	                               /* one-rank all-reduce: exercises the RCCL path on a one-GPU box; default: host sum)   */
	uint32_t counting_variant;     /* counting / capturing scanners: 0 default = whole text lines per lane and entries     */
	                               /* that are LDS addresses (CountingRowKernel: rows indexed by the byte for tables of up */
	                               /* to 64 states, by the table's letters for any other whose rows fit the LDS; up to 8   */
	                               /* regexps) for batches that fill the GPU, else 16 bytes of text at a time and 16-bit   */
	                               /* entries / the 32-bit kernel; 1 always the latter; 2 the former whenever the table    */
	                               /* fits.  Same results either way.                                                      */
	uint32_t slow_stats;           /* 1: every SlowScanner call prints to stderr how many strings left the list kernel     */
	                               /* (synchronises the stream: measurements)                                              */
	uint32_t walk_variant;         /* fixed-length records of tables with more states than dense rows: 0 default = the     */
	                               /* class-indexed walk (every row of the first ~1 700 states of the ranking in LDS, the  */
	                               /* reference's two-lookup step, multi.h:169-192) once the share of the scans' steps     */
	                               /* outside the 255 dense rows passes 0.05 % (measured by adapt(); 5 % of the a-priori   */
	                               /* estimate before), else the dense rows; 1 always the dense rows; 2 always the         */
	                               /* class-indexed walk with one string per lane, 3 always with two strings per lane      */
	                               /* (twice the table loads on their way beyond the rows, half the waves); 0 takes two    */
	                               /* for batches that give every wave slot of the chip a task of 128 strings (2^19 on    */
	                               /* 256 CUs).  Same results either way.                                                  */
	uint32_t selftest;             /* the first time a table takes one of the kernels of pire_hip_run[_strided] (dense     */
	                               /* rows, class-indexed walk, one string per lane, stream) that kernel first scans a     */
	                               /* known-answer batch of 256 x 512 bytes -- text that walks this table's own states --  */
	                               /* and the library compares it with the host image's transitions (pire_hip_table_next): */
	                               /* a mismatch returns PIRE_HIP_ESELFTEST and nothing is written.  The kernels keep text */
	                               /* on its way in registers with hand-counted waits; this catches a build or a device    */
	                               /* on which that goes wrong where the build-time ISA audit (pire_hip_build_info) only   */
	                               /* argues that it cannot.  ~1 ms once per table and kernel, on a stream of its own      */
	                               /* (an ON_DEVICE call blocks for that long, once); skipped while `stream` is being      */
	                               /* captured.  0 default = on; 1 off; 2 on, with the expected answer of one string        */
	                               /* altered (tests of the failure path)                                                  */
	uint32_t zip_variant;          /* the class-indexed walk's LDS image: 0 default = ZIPPED (a row of their own only for   */
	                               /* <= 1 022 states; every other state of the tier 10 bytes: the row it is equal to       */
	                               /* except in <= 3 letters, and where those lead -- 8-10 000 states of a dictionary        */
	                               /* scanner in a CU's LDS instead of 2 200, two dependent LDS reads per byte instead of   */
	                               /* one) once adapt() has measured more than 0.4 % of the steps outside the plain rows     */
	                               /* and the zipped tier leaves less than 0.6 of that outside; 1 never; 2 whenever the     */
	                               /* table has more states than plain rows.  Read when a table is ranked (created,          */
	                               /* adapted).  Same results either way.                                                    */
} pire_hip_config;
#define PIRE_HIP_SEGMENT_WARMUP_NONE (~(uint64_t)0)
#define PIRE_HIP_SEGMENT_BUDGET_NONE (~(uint64_t)0)

/* What this library is: the compiler its kernels' ISA audits passed with and the units they looked at -- or that it is
 * not the audited product build.  The kernels that keep text on its way in registers rely on what hipcc emits for them
 * (no spill, no copy of a register a load still owes data to); `make` checks that for every build and does not link a
 * library that fails (pire_amd/csrc/Makefile, tools/audit/build_audit.py). */
const char* pire_hip_build_info(void);

/* Copies min(out->size, sizeof) bytes of the current configuration; out->size must be set by the caller. */
int pire_hip_config_get(pire_hip_config* out);
/* Replaces the configuration (fields beyond in->size keep their current values). */
int pire_hip_config_set(const pire_hip_config* in);

/* Geometry of an ingested scanner; mirrors the public getters of Pire::Scanner. */
typedef struct pire_hip_table_info {
	uint32_t abi_version;
	uint32_t states;          /* Scanner::Size()          multi.h:134 */
	uint32_t letters;         /* Scanner::LettersCount()  multi.h:140 */
	uint32_t regexps;         /* Scanner::RegexpsCount()  multi.h:139 */
	uint32_t initial;         /* StateIndex(Initialize()) multi.h:161, 281-284 */
	uint32_t empty;           /* Scanner::Empty()         multi.h:135 */
	uint32_t header_size;     /* HEADER_SIZE in transitions, multi.h:349 (18 for Scanner, 2 for ScannerNoMask) */
	uint32_t row_stride;      /* RowSize()*sizeof(Transition) of the RELOCATABLE form, multi.h:347 */
	uint32_t hot_states;      /* states resident in LDS as dense 256-column rows (device layout) */
	uint32_t lds_table_bytes; /* LDS bytes the table occupies per workgroup */
	uint64_t device_bytes;    /* HBM bytes of the device-side table */
	uint64_t ref_buf_size;    /* Scanner::BufSize()       multi.h:297-305 */
	uint64_t last_trap_samples; /* cold-state samples seen by the most recent pire_hip_table_adapt() */
	uint32_t adaptations;     /* how many times pire_hip_table_adapt() changed the LDS rows */
	uint32_t compact_states;  /* states (hot ones included) that also have a class-indexed u16 row in LDS: the
	                             exact re-walk of a chunk that left the dense rows stays in LDS for them */
	uint32_t scanner_type;    /* ScannerIOTypes of the ingested blob (scanners/common.h:34-40): 1 Scanner, 2 SimpleScanner */
	uint32_t zip_full_states; /* != 0: the wide walk's image is zipped (pire_hip_config.zip_variant) and this many of its   */
	                          /* wide_states have a row of their own                                                     */
	uint32_t wide_states;     /* states with a class-indexed row in the wide walk's LDS image (0: table fits the dense rows) */
	uint32_t wide_lds_bytes;  /* LDS bytes of that image per workgroup */
	float outside_dense_share;   /* share of the ranking's mass (scans seen by adapt(), else the a-priori byte model) on   */
	                             /* states without a dense row                                                             */
	float outside_wide_share;    /* ... without a row of the class-indexed walk.  Once that walk has run: the share of the */
	                             /* steps of the scans between the two most recent adapt() calls that it SAW outside its    */
	                             /* rows (of its visit samples, one lane per wave and 128-byte tile, those that found their */
	                             /* lane there) -- not a share of the ranking's mass, which only knows states some sample   */
	                             /* hit                                                                                     */
	uint32_t shares_measured;    /* 1: those shares come from visit counters                                               */
	float zip_outside_share;     /* the plan that chose between the two images (last ranking): share of the ranking's mass  */
	                             /* the zipped tier would leave outside (0: not planned) ...                               */
	uint64_t last_wide_trap_chunks; /* 16-byte wave-chunks (64 strings x 16 bytes) the class-indexed walk had to walk a    */
	                                /* second time because a lane left its rows, between the two most recent adapt() calls  */
	                                /* (exact, all devices)                                                                 */
	float wide_outside_chunk_share; /* ... as a share of the wave-chunks that walk was handed in that time (a wave that skips */
	                                /* the attempt on the rows alone counts the chunks in which a lane left them)           */
	float zip_plain_outside_share; /* ... and the plain rows                                                               */
} pire_hip_table_info;

/* ---- table life cycle -------------------------------------------------------------------------- */

/*
 * Ingest a scanner from the bytes written by Pire::Scanner::Save() / NonrelocScanner::Save()
 * (multi.h:557-573; a Nonreloc scanner serialises as Relocatable, multi.h:604-608) or by
 * Pire::SimpleScanner::Save() (scanner_io.cpp:35-49; dense rows without letter classes, one regexp, never Dead --
 * its columns are folded into letter classes here, results are identical).  Replaces
 * Scanner::Load (multi.h:575-599) / Scanner::Mmap (multi.h:244-279) for the GPU side.  Validates the
 * header like Header::Validate.  The blob is copied; the handle is immutable and may be shared between
 * host threads.  Works without a GPU (host-side parse only); the device image is uploaded on first run
 * or by pire_hip_table_upload().
 */
int pire_hip_table_create(const void* save_blob, size_t len, pire_hip_table** out);

/*
 * Scanner::Mmap / SimpleScanner::Mmap twin (multi.h:244-279, simple.h:120-151): ingest the scanner at the start
 * of a mapped image and report in *consumed (nullable) how many bytes it occupied -- the offset of the pointer
 * Mmap() returns -- so that images holding several scanners back to back can be walked.  The image is decoded,
 * not aliased: it may be unmapped as soon as the call returns.
 */
int pire_hip_table_mmap(const void* image, size_t size, pire_hip_table** out, size_t* consumed);

/* Map `path` read-only and ingest its first scanner: the deployment flow of samples/blacklist/blacklist.cpp:64-93
 * (compile once with Scanner::Save, mmap everywhere). */
int pire_hip_table_create_from_file(const char* path, pire_hip_table** out);

/*
 * Scanner::Glue(lhs, rhs, maxSize) (multi.h:1092-1103) on two ingested Pire::Scanner tables, host side, without the
 * reference library: the product automaton with the reference's own letter classes (glue.h:35-46, 123-127), the
 * reference's own breadth-first state numbering (determine.h:91-137) -- so StateIndex values are identical to those
 * of the scanner the reference would glue -- and its flags / AcceptedRegexps lists (rhs ids shifted by
 * lhs.RegexpsCount(), multi.h:1024-1043).  max_size 0 = the reference's default 80 000.  As in the reference an
 * empty lhs (rhs) returns a copy of rhs (lhs), and exceeding max_size yields an EMPTY scanner (info.empty = 1), not
 * an error.  The result is a table like any other: run it, adapt it, glue it further.
 */
int pire_hip_table_glue(const pire_hip_table* lhs, const pire_hip_table* rhs, size_t max_size, pire_hip_table** out);
/*
 * The same product, with the state discovery (Impl::Determine's loop, determine.h:100-122) done on the GPU: a
 * level-synchronous breadth-first search over state pairs whose new states are numbered by the position of their
 * first occurrence inside the level -- which is exactly the order in which the sequential reference loop meets them,
 * so the result is identical to pire_hip_table_glue() and to the scanner the reference would glue.  Needs a HIP
 * device (PIRE_HIP_ENODEVICE otherwise).  Worth it for large products (tens of thousands of states).
 */
int pire_hip_table_glue_gpu(const pire_hip_table* lhs, const pire_hip_table* rhs, size_t max_size, pire_hip_table** out);

/*
 * This table's own configuration: from now on every entry point that takes `t` runs under *cfg instead of the process-wide
 * configuration (pire_hip_config_set) -- kernel routing, walk / zip variants at its next ranking, the adaptation policy, the
 * first-use self-test --, on whatever thread it is called.  Two users of the library in one process need not agree on the
 * process-wide knobs (or touch them at all).  cfg == NULL: back to the process-wide configuration.  Fields beyond cfg->size take
 * the process-wide values of the moment of the call.  Waits for calls in flight on `t` (not for the device).
 * pire_hip_run_pair on two tables with configurations of their own: the first table's.
 */
int pire_hip_table_config_set(pire_hip_table* t, const pire_hip_config* cfg);
/* The configuration calls on `t` run under (its own, else the process-wide one); out->size as pire_hip_config_get. */
int pire_hip_table_config_get(const pire_hip_table* t, pire_hip_config* out);

/* Upload the device image to the CURRENT HIP device now (otherwise done lazily by the first run). */
int pire_hip_table_upload(pire_hip_table* t);

/*
 * Re-rank the LDS-resident dense rows from what the scans on this table actually visited (the kernels keep
 * sampled visit counters on the device).  A table is created with rows ranked by a byte model of "typical"
 * text; after a representative batch, adapt() promotes the states the data really spends its time in, so that
 * later batches stay on the one-LDS-gather-per-byte path.  Purely a performance call: results are bit-exact
 * with or without it.  Synchronises the device; must not run concurrently with scans on the same table.
 * *changed_rows (nullable) receives the number of rows that entered the dense set.
 */
int pire_hip_table_adapt(pire_hip_table* t, uint32_t* changed_rows);

/*
 * The checked build of the scan kernel (pire_hip_config.checked = 1; the analogue of the reference's
 * ValidateSkip, multi.h:925-934, which re-walks what the exit masks skipped): the wave-wide early-out on absorbing
 * states is only noted, the text is walked to its end all the same, and every lane whose state still moved after its
 * wave had been declared absorbing is counted.  *out receives the count since the last call (0 = the early-out was
 * result-neutral, as it must be) and the counter is cleared.  Synchronises the devices the table ran on.
 */
int pire_hip_table_check_failures(pire_hip_table* t, uint64_t* out);

void pire_hip_table_destroy(pire_hip_table* t);

int pire_hip_table_get_info(const pire_hip_table* t, pire_hip_table_info* out);
/* pire_hip_table_info has no size field and has grown at its end between ABI versions: a caller built against an older header
 * passes ITS sizeof and gets the fields it knows (min(size, sizeof) bytes are written) -- or checks pire_hip_abi_version(), what
 * the loaded library was built as, against its own PIRE_HIP_ABI_VERSION before calling pire_hip_table_get_info. */
int pire_hip_table_get_info_sized(const pire_hip_table* t, void* out, size_t size);
uint32_t pire_hip_abi_version(void);

/* ---- per-state queries on the host (no GPU involved) ------------------------------------------- */

/* Scanner::Final(state)  multi.h:143.   idx = StateIndex. Returns 0/1, or <0 on bad idx. */
int pire_hip_table_final(const pire_hip_table* t, uint32_t state_idx);
/* Scanner::Dead(state)   multi.h:147 */
int pire_hip_table_dead(const pire_hip_table* t, uint32_t state_idx);
/* Scanner::AcceptedRegexps(state) multi.h:149-158: (begin, count) describe an array owned by the table, valid until
 * pire_hip_table_destroy(t) whatever re-rankings (pire_hip_table_adapt, the automatic ones) happen in between. */
int pire_hip_table_accepted_regexps(const pire_hip_table* t, uint32_t state_idx,
                                    const uint64_t** begin, size_t* count);
/* The letter class of ch (Translate(ch) - HEADER_SIZE, multi.h:163-166); ch < 264. */
int pire_hip_table_letter_class(const pire_hip_table* t, uint32_t ch);
/*
 * Scanner::Next (multi.h:189-192) as a TABLE ACCESSOR on state indices: the index reached from state_idx on
 * ch (ch < 260, ch != 257), or <0.  For inspecting an ingested table and for single Step()s on one host-side
 * state (RunHelper::Step, run.h:371); it is not, and must not be used as, a scan loop -- Run() is GPU only.
 */
int64_t pire_hip_table_next(const pire_hip_table* t, uint32_t state_idx, uint32_t ch);
/*
 * Device-layout introspection (tests): orig_of_perm[states] = reference state index of
 * each device ("perm") id; hot_rows[(hot_states+1)*256] = the dense LDS rows, entries are perm ids < hot_states
 * or hot_states (= trap: the lane leaves the LDS-resident set).  Either pointer may be NULL.
 */
int pire_hip_table_layout(const pire_hip_table* t, uint32_t* orig_of_perm, uint8_t* hot_rows);
/*
 * ... and of the class-indexed walk's LDS image (pire_hip_config.walk_variant; tables with more states than dense rows):
 * *wide_states device ids [0, wide_states) have a row, *pitch bytes apart, the first at LDS byte address *rows_offset;
 * rows[(wide_states + 1) * pitch / 2] (cap = its capacity in u16 entries; NULL: only the geometry): per row `letters`
 * entries = the device id of the target state (wide_states, the id of the last row -- the escape row, which leads to
 * itself -- for targets without a row), then the row's flags (1 Final, 2 Dead, 4 every transition a self loop).
 * wide_states == 0: no such image.
 */
int pire_hip_table_wide_layout(const pire_hip_table* t, uint16_t* rows, size_t cap, uint32_t* wide_states, uint32_t* pitch,
                               uint32_t* rows_offset);
/*
 * ... and of its ZIPPED form (pire_hip_config.zip_variant; pire_hip_table_wide_layout reports wide_states = 0 for such a table).
 * geometry[8] = { tier, full, pitch, rows_offset, headers_offset, exceptions_offset, image_end, 3 }: device ids [0, full) have a
 * row of their own (as above, `tier` = the escape state's id, row number `full` = the escape row), ids [full, tier) a header and
 * three exception targets; all zeros: the table's image is not zipped.  image[(image_end - rows_offset) / 2] (cap = its capacity
 * in u16 entries; NULL: only the geometry) = the bytes as they lie in LDS from rows_offset on:
 *     rows              (full + 1) x pitch bytes
 *     u32 header[tier + 1]  at headers_offset: bits 22..31 the row (device id < full, or `full`) this state's row is equal to except
 *                       in the letters at bits 1..7, 8..14, 15..21 (127 = none)
 *     u16 target[tier - full][3]  at exceptions_offset: where those letters lead (device id, `tier` = outside the tier)
 */
int pire_hip_table_zip_layout(const pire_hip_table* t, uint16_t* image, size_t cap, uint32_t geometry[8]);

/* ---- the hot path -------------------------------------------------------------------------------- */

/*
 * For each i in [0,n):   st = Initialize() or state #init_state_idx[i]       (RunHelper ctors, run.h:368-369)
 *                        if (flags & BEGIN) Step(st, BeginMark)
 *                        Run(st, text + offsets[i], text + offsets[i+1])    (Pire::Run, run.h:271-275)
 *                        if (flags & END)   Step(st, EndMark)
 *                        out_state_idx[i] = StateIndex(st);  out_final[i] = Final(st)
 * out_counts (nullable), uint64[regexps + 2], is ACCUMULATED into (caller zeroes it):
 *     [0] += number of strings whose end state is Final,  [1] += n,
 *     [2 + r] += number of strings whose end state lists regexp r in AcceptedRegexps().
 * init_state_idx, out_state_idx, out_final may each be NULL.  n == 0, zero-length strings and the empty
 * scanner are valid (tests/pire_ut.cpp:760-837).  Offsets are byte offsets into text, non-decreasing.
 * `stream` is a hipStream_t (NULL = default stream).
 *
 * Few long strings (strings of 8 KiB or more on average, too few of them to keep the lanes busy) are cut into
 * segments that are scanned in parallel from guessed start states; the chain of segments is then composed on the
 * device and only results computed from the true state are accepted, so the answers are the same
 * (pire_amd/csrc/segmented.hip: one 1 GiB string in 0.54 ms instead of 45 s).  The host has to know the lengths for
 * that: host pointers, pire_hip_run_strided, PIRE_HIP_RUN_HOST_OFFSETS -- and, for offsets that live on the device, a
 * batch of fewer than 65 536 strings is PEEKED at: its first and last offset are read back (which synchronises
 * `stream`), and all of them only if the segmented scan is then chosen (pire_hip_config.no_offsets_peek = 1 keeps such
 * calls enqueue-only).  A segmented call synchronises `stream` even with PIRE_HIP_RUN_ON_DEVICE.
 * PIRE_HIP_RUN_GENERIC (or pire_hip_config.no_segments) keeps one string per lane.
 */
int pire_hip_run(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n,
                 uint32_t flags, const uint32_t* init_state_idx,
                 uint32_t* out_state_idx, uint8_t* out_final, uint64_t* out_counts, void* stream);

/*
 * Same walk over fixed-length records: string i = text[i*stride, i*stride + len).  This is the layout the
 * tiled LDS-resident kernel is specialised for: stride a multiple of 16, text 16-byte aligned, len >= 128 (any
 * len: what the whole 128-byte tiles leave of a record is walked byte by byte), n >= 64, 64 * stride < 2^31;
 * anything else is routed to the generic kernel with the same results.  Bytes behind a record's len, up to its
 * stride, are never walked.
 */
int pire_hip_run_strided(pire_hip_table* t, const void* text, uint64_t n, uint64_t len, uint64_t stride,
                         uint32_t flags, const uint32_t* init_state_idx,
                         uint32_t* out_state_idx, uint8_t* out_final, uint64_t* out_counts, void* stream);

/*
 * Pire::Step (run.h:50-57) on a device-resident array of state indices: state_idx[i] = Next(state_idx[i], ch),
 * ch < 260 (bytes, BeginMark 258, EndMark 259).  Device pointers only.
 */
int pire_hip_step(pire_hip_table* t, uint32_t* state_idx, uint64_t n, uint32_t ch, void* stream);

/* ---- which strings matched which regexps, on the device --------------------------------------------------- */

/* W = max(1, ceil(RegexpsCount() / 64)): the number of 64-bit words of a regexp mask of this table (0: null table). */
uint32_t pire_hip_table_mask_words(const pire_hip_table* t);

/*
 * From end states to matches.  state_idx[i] is a StateIndex as pire_hip_run writes it (reference numbering).
 *   mask(i)[w] bit b  <=>  regexp 64*w + b is in AcceptedRegexps(state_idx[i])   (multi.h:149-158)
 *   selected(i)       <=>  want == NULL ? Final(state_idx[i]) : (mask(i) & want) != 0     (want: W words; bits at or
 *                          above RegexpsCount() are ignored; a scanner with 0 regexps selects nothing)
 * out_masks     (nullable) [n][W]   mask(i) of every string
 * out_hits      (nullable) [hit_cap] the indices i of the selected strings, ASCENDING
 * out_hit_masks (nullable) [hit_cap][W] mask of out_hits[k]
 * out_hit_count (required) *count = number of selected strings, also when it exceeds hit_cap; only the first
 *               min(count, hit_cap) entries of out_hits / out_hit_masks are written, nothing behind them
 * n == 0 writes a count of 0.  n < 2^32.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> every pointer (want included) is a device pointer and the call only enqueues on
 *        `stream`: three small kernels whose per-call scratch (n / 8 + n / 256 bytes) comes from the stream-ordered
 *        allocator (hipMallocAsync / hipFreeAsync on `stream`), as the row kernels' does (see pire_hip_run_half_final):
 *        enqueue-only, and legal inside a stream capture under the same condition as those calls -- not something every
 *        capture mode accepts.  The first call on a device uploads the table's mask image (W words and the Final flag
 *        per state, by reference state index -- no re-ranking touches it) synchronously; pire_hip_table_upload()
 *        beforehand does that too.  A state_idx[i] >= Size() is undefined in this mode.
 *        Otherwise host pointers: staged, synchronises; a state_idx[i] >= Size() is PIRE_HIP_EINVAL.
 * PIRE_HIP_EINVAL before any device is touched: null table, n with a null state_idx, null out_hit_count, hit_cap > 0
 * with null out_hits, out_hit_masks without out_hits.
 * pire_hip_last_kernel() is not changed by the select pass: it keeps naming the scan kernel.
 */
int pire_hip_select(pire_hip_table* t, const uint32_t* state_idx, uint64_t n, const uint64_t* want, uint32_t flags,
                    uint64_t* out_masks, uint64_t* out_hits, uint64_t* out_hit_masks, uint64_t hit_cap,
                    uint64_t* out_hit_count, void* stream);

/*
 * pire_hip_run / pire_hip_run_strided followed by pire_hip_select behind one call, on the same stream.  The first
 * arguments, the flags (BEGIN / END / ON_DEVICE / GENERIC / HOST_OFFSETS / NO_PEEK) and out_state_idx / out_final /
 * out_counts (each nullable) are the run calls'; the rest pire_hip_select's.  With out_state_idx == NULL the state indices
 * live in scratch of the library's own (stream-ordered in ON_DEVICE mode).  In host-pointer mode the hit indices are
 * relative to the whole batch, whatever chunks the staging cut it into.  With PIRE_HIP_RUN_HOST_OFFSETS only `offsets`
 * is a host pointer; what makes the run call wait makes this one wait.
 */
int pire_hip_run_select(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                        const uint32_t* init_state_idx, uint32_t* out_state_idx, uint8_t* out_final, uint64_t* out_counts,
                        const uint64_t* want, uint64_t* out_masks, uint64_t* out_hits, uint64_t* out_hit_masks,
                        uint64_t hit_cap, uint64_t* out_hit_count, void* stream);
int pire_hip_run_select_strided(pire_hip_table* t, const void* text, uint64_t n, uint64_t len, uint64_t stride, uint32_t flags,
                                const uint32_t* init_state_idx, uint32_t* out_state_idx, uint8_t* out_final,
                                uint64_t* out_counts, const uint64_t* want, uint64_t* out_masks, uint64_t* out_hits,
                                uint64_t* out_hit_masks, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);

/* ---- one hit list per regexp, on the device --------------------------------------------------------------- */

/*
 * From end states to the question a multi-rule caller asks: for EVERY regexp r of a glued scanner, the ascending list of
 * the strings that matched r, in one pass.  R = RegexpsCount(); state_idx[i] as for pire_hip_select.
 *   member(i, r)  <=>  r is in AcceptedRegexps(state_idx[i]) (multi.h:149-158) and r < R   (the mask image of
 *                      pire_hip_select: reference state numbering, untouched by re-rankings)
 * out_hit_counts (required when R > 0) [R]  out_hit_counts[r] = the number of i with member(i, r), the full count also
 *                where it exceeds hit_cap; every one of the R entries is written, zeros included
 * out_hits       (nullable when hit_cap == 0) [R][hit_cap]  row r = the indices i with member(i, r), ASCENDING; only the
 *                first min(out_hit_counts[r], hit_cap) entries of a row are written, nothing behind them, in that row or
 *                any other.  A string that matches k regexps appears in k rows.
 * The pitch is fixed so that the rows chain into R gathers with device pointers and no read-back: row r is
 * pire_hip_gather(.., idx = out_hits + r * hit_cap, idx_count = out_hit_counts + r, idx_cap = hit_cap, ..).
 * n == 0 writes R zero counts.  R == 0 returns PIRE_HIP_OK and writes nothing.  n >= 2^32: PIRE_HIP_EUNSUPPORTED.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> every pointer is a device pointer and the call only enqueues on `stream`: three
 *        kernels (count per tile and regexp, R scans, scatter), no atomics -- the same input gives the same bits.  The
 *        per-call scratch (4 * R * ceil(n / 1024) bytes) comes from the stream-ordered allocator (hipMallocAsync /
 *        hipFreeAsync on `stream`), as pire_hip_select's does: enqueue-only, and legal inside a stream capture under the
 *        same condition as that call -- not something every capture mode accepts.  The first call on a device uploads the
 *        table's mask image synchronously (pire_hip_select's; pire_hip_table_upload() beforehand does that too).  A
 *        state_idx[i] >= Size() is undefined in this mode for the caller; it reads nothing and is a member of no row.
 *        Otherwise host pointers: staged, synchronises; a state_idx[i] >= Size() is PIRE_HIP_EINVAL.  The rows are staged
 *        at a pitch of min(hit_cap, n) and come back one by one, only their written entries; the caller's pitch stays
 *        hit_cap.
 * PIRE_HIP_EINVAL before any device is touched: null table, n with a null state_idx, null out_hit_counts (R > 0),
 * hit_cap > 0 with null out_hits.
 * pire_hip_last_kernel() is not changed by the pass: it keeps naming the scan kernel.  No first-use self-test (as
 * pire_hip_select).
 */
int pire_hip_route(pire_hip_table* t, const uint32_t* state_idx, uint64_t n, uint32_t flags, uint64_t* out_hits,
                   uint64_t hit_cap, uint64_t* out_hit_counts, void* stream);

/*
 * pire_hip_run / pire_hip_run_strided followed by pire_hip_route behind one call, on the same stream.  The first
 * arguments, the flags and out_state_idx / out_final / out_counts (each nullable) are the run calls'; the rest
 * pire_hip_route's.  With out_state_idx == NULL the state indices live in scratch of the library's own (stream-ordered in
 * ON_DEVICE mode).  In host-pointer mode the indices of the whole batch arrive in one array before the pass: hit indices
 * are relative to the whole batch, whatever chunks the staging cut it into.  R == 0: the scan runs, the pass writes nothing.
 */
int pire_hip_run_route(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                       const uint32_t* init_state_idx, uint32_t* out_state_idx, uint8_t* out_final, uint64_t* out_counts,
                       uint64_t* out_hits, uint64_t hit_cap, uint64_t* out_hit_counts, void* stream);
int pire_hip_run_route_strided(pire_hip_table* t, const void* text, uint64_t n, uint64_t len, uint64_t stride, uint32_t flags,
                               const uint32_t* init_state_idx, uint32_t* out_state_idx, uint8_t* out_final,
                               uint64_t* out_counts, uint64_t* out_hits, uint64_t hit_cap, uint64_t* out_hit_counts,
                               void* stream);

/* ---- raw text into strings, on the device ------------------------------------------------------------------- */

/* The split pass cuts raw into tiles of this many bytes, on the 16-byte grid of raw's address (tests aim at its edges). */
#define PIRE_HIP_SPLIT_TILE_BYTES 16384u

/*
 * Where the strings of a delimited buffer are: the step in front of every scan call, which wants text + offsets[n + 1]
 * with nothing between the strings.  getline's semantics: the strings are the runs between delimiter bytes; the delimiter
 * is not part of a string; a trailing fragment without a delimiter is a string; a buffer that ends in a delimiter has no
 * extra empty string behind it; an empty buffer has no strings; consecutive delimiters give empty strings.  With D
 * delimiter bytes in raw[0, size), the k-th of them (from 1) at p_k:
 *   n = D + (size > 0 && raw[size - 1] != delim)
 *   out_offsets[0] = 0,  out_offsets[k] = p_k - (k - 1) for 1 <= k <= D,  out_offsets[n] = size - D
 *   out_text = raw without its delimiter bytes, size - D bytes (room for `size` bytes is always enough)
 * so string i is out_text[out_offsets[i], out_offsets[i + 1]) and, in the buffer it came from,
 *   raw[out_offsets[i] + i, out_offsets[i + 1] + i).
 * out_text == NULL: nothing is copied, the offsets index raw itself and every string keeps its delimiter as its last
 * byte: out_offsets[k] = p_k + 1, out_offsets[n] = size (for callers whose scanner tolerates the delimiter).
 * out_n (required) receives n, also when n > offsets_cap.  out_offsets (nullable when offsets_cap == 0) has
 * offsets_cap + 1 entries; only entries 0..min(n, offsets_cap) are written, nothing behind them.  size == 0 writes
 * n = 0 and out_offsets[0] = 0.  delim is a byte value.  The pass is not in-place.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> every pointer is a device pointer and the call only enqueues on `stream`: three
 *        kernels (count per tile, one-block scan, scatter), no atomics -- the same input gives the same bits --, 12 bytes
 *        of scratch per tile from the stream-ordered allocator.  raw and out_text may have any alignment.
 *        Otherwise host pointers: staged, synchronises.
 * PIRE_HIP_EINVAL before any device is touched: delim > 255, null out_n, size > 0 with null raw, offsets_cap > 0 with
 * null out_offsets, out_text[0, size) overlapping raw[0, size).
 */
int pire_hip_split(const void* raw, uint64_t size, uint32_t delim, uint32_t flags, void* out_text, uint64_t* out_offsets,
                   uint64_t offsets_cap, uint64_t* out_n, void* stream);

/*
 * Raw bytes in, the matching lines out: pire_hip_split into scratch of the library's own, pire_hip_run_select on the
 * result, and one small kernel that turns the hit list into byte ranges of the raw buffer.
 * out_line_count (required)  n, the number of lines
 * out_hits       (nullable)  [hit_cap] the numbers (from 0) of the selected lines, ascending
 * out_hit_spans  (nullable)  [hit_cap][2] begin, end: hit k is raw[begin, end), its delimiter not included
 * out_hit_masks  (nullable)  [hit_cap][W]
 * want, hit_cap, out_hit_count (required): exactly pire_hip_select's; out_hit_spans and out_hit_masks need out_hits.
 * flags: PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END | PIRE_HIP_RUN_GENERIC | PIRE_HIP_RUN_ON_DEVICE (every pointer a device
 * pointer).  The call reads n back (8 bytes) between the split's scan and its scatter, to size the offsets: it
 * synchronises `stream` once EVEN WITH PIRE_HIP_RUN_ON_DEVICE, and what it enqueues behind that is enqueue-only.
 * PIRE_HIP_EINVAL before any device is touched: what pire_hip_select refuses, delim > 255, null out_line_count,
 * size > 0 with null raw.  pire_hip_last_kernel() names the scan kernel.  Fewer than 2^32 lines.
 */
int pire_hip_run_lines_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                              const uint64_t* want, uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans,
                              uint64_t* out_hit_masks, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);

/*
 * Raw bytes in, the matching lines of every regexp out: the split and the scan of pire_hip_run_lines_select, then
 * pire_hip_route on the lines and one small kernel that turns all rows into byte ranges of the raw buffer.
 * out_line_count (required)  n, the number of lines
 * out_hits, hit_cap, out_hit_counts: exactly pire_hip_route's, the indices being line numbers (from 0)
 * out_hit_spans  (nullable, needs out_hits) [R][hit_cap][2]  begin, end: hit k of row r is raw[begin, end), its delimiter
 *                not included, exactly as in pire_hip_run_lines_select; written as far as the row's hits are.  The layout
 *                makes pire_hip_gather_spans(raw, size, out_hit_spans + 2 * r * hit_cap, out_hit_counts + r, hit_cap, ..)
 *                legal with device pointers and no read-back.
 * flags as pire_hip_run_lines_select.  The call reads n back to size the offsets: it synchronises `stream` once EVEN WITH
 * PIRE_HIP_RUN_ON_DEVICE, at the same place and for the same reason as pire_hip_run_lines_select, and adds no second
 * wait.  size == 0: n = 0 and R zero counts.  R == 0: n is written, nothing else.
 * PIRE_HIP_EINVAL before any device is touched: what pire_hip_route refuses, out_hit_spans without out_hits, delim > 255,
 * null out_line_count, size > 0 with null raw.  pire_hip_last_kernel() names the scan kernel.  Fewer than 2^32 lines.
 */
int pire_hip_run_lines_route(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                             uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans, uint64_t hit_cap,
                             uint64_t* out_hit_counts, void* stream);

/* ---- the selected strings gathered into a batch, on the device ------------------------------------------------ */

/* The copy pass cuts out_text into tiles of this many bytes, on the 16-byte grid of out_text's address (tests aim at its edges). */
#define PIRE_HIP_GATHER_TILE_BYTES 16384u
#define PIRE_HIP_GATHER_NO_TAIL (~0u)

/*
 * From a hit list to bytes: the listed strings of a batch, back to back, as text + offsets -- the input form of every scan
 * entry point, so that a second scanner runs on the survivors of a first one without the text leaving the device; with a
 * tail byte behind every string it is grep's output buffer, and the inverse of pire_hip_split.
 *   k   = min(idx_count ? *idx_count : idx_cap, idx_cap)               the number of strings copied
 *   s_j = idx ? idx[j] : j                    for j < k                 the source of output string j:
 *                                                                       text[offsets[s_j], offsets[s_j + 1])
 *   a   = (tail != PIRE_HIP_GATHER_NO_TAIL)                             one byte `tail` behind every string, or none
 *   L_j = offsets[s_j + 1] - offsets[s_j] + a
 *   out_offsets[0] = 0,  out_offsets[j + 1] = L_0 + ... + L_j
 *   out_text[out_offsets[j], out_offsets[j + 1]) = the string, then the byte `tail` if a
 *   *out_bytes = out_offsets[k]
 * idx need not be ascending or distinct (the hit lists of pire_hip_select are; a caller's own order is legal).  With a tail
 * every output string keeps it as its last byte: the convention of pire_hip_split's out_text == NULL form.
 * out_bytes (required) receives the whole total, also when it exceeds text_cap; only bytes of out_text at positions
 * < text_cap are written, nothing behind them.  out_offsets has idx_cap + 1 entries; entries 0..k are written, nothing
 * behind them.  idx_cap == 0 or k == 0 writes *out_bytes = 0 and out_offsets[0] = 0 (where out_offsets is not null).
 * idx_cap < 2^32.
 * pire_hip_gather_spans: the source of output string j is raw[spans[2j], spans[2j + 1]) -- what out_hit_spans of
 * pire_hip_run_lines_select holds; k and the rest as above with span_count / span_cap.  A range with end < begin or
 * end > size is out of range.
 * An index s_j >= n, or a span out of range: with host pointers PIRE_HIP_EINVAL and nothing is written; with
 * PIRE_HIP_RUN_ON_DEVICE it contributes an empty string (and its tail) and reads nothing.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> every pointer (idx_count included) is a device pointer and the call only enqueues on
 *        `stream`: four kernels (lengths per tile of 1 024 strings, one-block scan, offsets, copy), no atomics -- the same
 *        input gives the same bits --, and no allocation of any kind: the pass needs no scratch (the per-tile sums wait
 *        in entries of out_offsets that it overwrites last), so calls right behind one another on a busy stream only
 *        enqueue, each of them.  The copy
 *        pass divides its work by OUTPUT BYTES: a string of megabytes spreads over as many blocks as it has tiles, empty
 *        strings cost nothing.  Device text is read under the rule stated at PIRE_HIP_RUN_ON_DEVICE.  text, raw and
 *        out_text may have any alignment.
 *        Otherwise host pointers: staged, synchronises.
 * The pass is not in place: out_text must not overlap the source.  That is refused where the host can tell: in the spans
 * form (out_text[0, text_cap) against raw[0, size)) and with host pointers (against text[0, offsets[n])).
 * PIRE_HIP_EINVAL before any device is touched: null out_bytes, tail > 255 (and not PIRE_HIP_GATHER_NO_TAIL), idx_cap > 0
 * with null offsets (span_cap > 0 with null spans), idx_cap > 0 with null out_offsets, text_cap > 0 with null out_text,
 * idx_cap > n without idx, 2^32 strings or more, out_text overlaps the source.
 * pire_hip_last_kernel() is not changed by a gather.  No first-use self-test (as pire_hip_split).
 */
int pire_hip_gather(const void* text, const uint64_t* offsets, uint64_t n,
                    const uint64_t* idx, const uint64_t* idx_count, uint64_t idx_cap, uint32_t tail, uint32_t flags,
                    void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* stream);

int pire_hip_gather_spans(const void* raw, uint64_t size,
                          const uint64_t* spans, const uint64_t* span_count, uint64_t span_cap, uint32_t tail, uint32_t flags,
                          void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* stream);

/*
 * pire_hip_run_lines_select followed by the gather of the selected lines from raw, behind one call: raw bytes in, the
 * matching lines out AS BYTES.  With tail = delim the bytes in out_text are exactly what `grep` prints for the buffer.
 * out_line_count, want, out_hits (nullable: the library keeps the hit list to itself), hit_cap, out_hit_count: as
 * pire_hip_run_lines_select; k = min(*out_hit_count, hit_cap) lines are gathered.  out_text, text_cap, out_offsets
 * (hit_cap + 1 entries), out_bytes: as pire_hip_gather.  flags as pire_hip_run_lines_select; it synchronises `stream`
 * once, for the same reason and at the same place, and adds no second wait.  It refuses what pire_hip_run_lines_select
 * refuses (hit_cap > 0 with null out_hits excepted) and what pire_hip_gather refuses of its outputs.
 * pire_hip_last_kernel() names the scan kernel.
 */
int pire_hip_run_lines_gather(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                              const uint64_t* want, uint32_t tail, uint64_t* out_line_count,
                              uint64_t* out_hits, uint64_t hit_cap, uint64_t* out_hit_count,
                              void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* stream);

/* ---- one column of every string, on the device ------------------------------------------------------------------- */

/* The fields pass cuts text into tiles of this many bytes, on the 16-byte grid of text's address (tests aim at its edges). */
#define PIRE_HIP_FIELDS_TILE_BYTES 16384u
#define PIRE_HIP_FIELDS_REST 0x1u        /* in `mode` */

/*
 * Where field `field` (from 0) of every string is: `awk -F sep '{print $(field + 1)}'` as byte ranges, the step between a
 * batch of records (access logs, TSV exports: what pire_hip_split hands back) and a scan of ONE column of them.
 * String i is text[offsets[i], offsets[i + 1]); offsets do not decrease.  It holds m bytes equal to `sep`, at positions
 * q_1 < ... < q_m (absolute in text); its m + 1 fields are the runs between them, so empty fields exist.  With
 * q_0 = offsets[i] - 1, q_{m+1} = offsets[i + 1] and k = field:
 *   k <= m:  out_spans[2i] = q_k + 1,  out_spans[2i + 1] = q_{k+1}
 *            mode & PIRE_HIP_FIELDS_REST:  out_spans[2i + 1] = offsets[i + 1] instead (`cut -f k-`: the last column of a
 *            log line may hold the separator)
 *   k >  m:  out_spans[2i] = out_spans[2i + 1] = offsets[i + 1]            (an empty span at the end of the string)
 * so an empty string gives an empty span at its offset.  Exactly 2n entries are written, nothing behind them; n == 0
 * writes nothing.  The spans are ranges of text:
 *   pire_hip_gather_spans(text, offsets[n], out_spans, NULL, n, PIRE_HIP_GATHER_NO_TAIL, ...)
 * is legal on them with device pointers (any size >= offsets[n] does: no read-back), and its output string i is the field
 * of input string i -- indices survive.  sep is a byte value.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> every pointer is a device pointer and the call only enqueues on `stream`: four kernels
 *        (defaults per string, count per tile, one-block carry, resolve).  The work is divided by BYTES -- tiles of
 *        PIRE_HIP_FIELDS_TILE_BYTES --: one line of megabytes, or a million empty ones, cost what their bytes cost.  The
 *        text is read twice.  No atomics -- the same input gives the same bits --, 16 bytes of scratch per block of the
 *        grid (at most 2 048 blocks, whatever the text holds) from the stream-ordered allocator.  text may have any
 *        alignment.
 *        Otherwise host pointers: staged, synchronises.
 * PIRE_HIP_EINVAL before any device is touched: sep > 255, unknown bits in mode, n > 0 with null offsets or null out_spans,
 * and with host pointers offsets that decrease and offsets[n] > 0 with null text.  PIRE_HIP_EUNSUPPORTED: n >= 2^32.
 * pire_hip_last_kernel() is not changed by the pass.  No first-use self-test (the pass takes no table, as pire_hip_split).
 */
int pire_hip_fields(const void* text, const uint64_t* offsets, uint64_t n, uint32_t sep, uint32_t field, uint32_t mode,
                    uint32_t flags, uint64_t* out_spans, void* stream);

/*
 * Raw bytes in, the lines whose COLUMN matches out: `awk -F sep '$(field + 1) ~ /re/'`.  pire_hip_run_lines_select with one
 * more step between its split and its scan: pire_hip_fields on the lines, pire_hip_gather_spans of the n fields into
 * scratch of the library's own, and the scan on THAT batch -- so PIRE_HIP_RUN_BEGIN / PIRE_HIP_RUN_END step the marks
 * around the field and an anchored pattern anchors to the column, and a match in another column selects nothing.  Hit k
 * of the scan is line k of raw: out_hits are line numbers and out_hit_spans the WHOLE lines in raw, delimiter not included.
 * A line with too few columns is scanned as the empty string.  sep, field, mode: as pire_hip_fields.
 * Everything else -- want, hit_cap, out_hit_count (the whole count, also beyond hit_cap), out_hit_masks, nothing written
 * behind the lists, the flags, the ONE synchronisation of `stream` (n read back between the split's scan and its scatter,
 * EVEN WITH PIRE_HIP_RUN_ON_DEVICE) -- is pire_hip_run_lines_select's.
 * PIRE_HIP_EINVAL before any device is touched: what pire_hip_run_lines_select refuses, sep > 255, sep == delim, unknown
 * bits in mode.  pire_hip_last_kernel() names the scan kernel.  Fewer than 2^32 lines.
 */
int pire_hip_run_lines_field_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t sep,
                                    uint32_t field, uint32_t mode, uint32_t flags, const uint64_t* want,
                                    uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans,
                                    uint64_t* out_hit_masks, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);

/*
 * pire_hip_run_lines_field_select followed by the gather of the selected WHOLE lines from raw: pire_hip_run_lines_gather
 * with the scan on one column.  tail, out_hits (nullable), out_text, text_cap, out_offsets, out_bytes: as there.
 */
int pire_hip_run_lines_field_gather(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t sep,
                                    uint32_t field, uint32_t mode, uint32_t flags, const uint64_t* want, uint32_t tail,
                                    uint64_t* out_line_count, uint64_t* out_hits, uint64_t hit_cap, uint64_t* out_hit_count,
                                    void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes,
                                    void* stream);

/*
 * Batched Runner over the table walked as a Pire::HalfFinalScanner (scanners/half_final.h:32-227).  A
 * HalfFinalScanner IS a Scanner (same Save() bytes, ingest it with pire_hip_table_create), but its Initialize and
 * every Step end with TakeAction, which counts, per regexp, the steps that end in a state final for it
 * (half_final.h:137-164): the number of -- possibly intersecting -- matches.  Per string i:
 *   out_results[i * RegexpsCount() + r] = State::Result(r)   (half_final.h:90-92; u32: a count is <= length + 3)
 *   out_state_idx / out_final (nullable)  = StateIndex / Final of the end state, as pire_hip_run.
 * flags: PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END | PIRE_HIP_RUN_ON_DEVICE (| PIRE_HIP_RUN_GENERIC: keep the
 * one-string-per-lane kernel; by default batches of >= 256 strings take the ragged kernel, which
 * re-walks exactly only the 16-byte chunks that touched a Final state).  PIRE_HIP_RUN_HOST_OFFSETS as for
 * pire_hip_run; few long strings of host-known length are counted segment-wise after the segmented scan has resolved
 * every segment's true start state.  Pinned by tests/count_ut.cpp:541-550, 575.
 * ON_DEVICE calls: what is said at PIRE_HIP_RUN_ON_DEVICE holds, with two additions.  Tables that count on the row kernel
 * (up to 8 regexps, rows that fit the LDS) keep a second image on the device: pire_hip_table_upload() uploads it with the
 * table; without that call the first pire_hip_run_half_final on a device allocates and copies it synchronously.  And a
 * call on the row kernel takes its per-call scratch (the length order of the strings, the list of strings whose counts
 * outgrow 16 bits) from the stream-ordered allocator (hipMallocAsync / hipFreeAsync on `stream`): enqueue-only, but
 * not something every capture mode accepts -- pire_hip_config.counting_variant = 1 keeps such calls off the row kernel.
 */
int pire_hip_run_half_final(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                            uint32_t* out_state_idx, uint8_t* out_final, uint32_t* out_results, void* stream);

/*
 * Pire::LongestPrefix / Pire::ShortestPrefix (run.h:277-311) for n strings: out_len[i] = length of the longest
 * (shortest) prefix of string i the scanner accepts, or -1 where the reference returns a null pointer.
 * through_begin / through_end as the reference's throughBeginMark / throughEndMark.  Scanning stops at the first
 * dead state (pire_ut.cpp:475-483).  flags: PIRE_HIP_RUN_ON_DEVICE, PIRE_HIP_RUN_GENERIC (as above).
 */
int pire_hip_prefix(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, int longest,
                    int through_begin, int through_end, uint32_t flags, int64_t* out_len, void* stream);

/*
 * Pire::Run(scanner1, scanner2, state1, state2, begin, end) (run.h:229-241) -- a Runner over
 * Pire::ScannerPair<Scanner1, Scanner2> (scanners/pair.h:33-94) -- for n strings: both scanners over the same text,
 *   out_state_idx1[i], out_state_idx2[i] = StateIndex of the two end states (pair.h:79-82),
 *   out_final[i] = Final(state1) || Final(state2)                            (pair.h:69-72).
 * Device pointers only (flags must carry PIRE_HIP_RUN_ON_DEVICE; BEGIN / END apply to both scanners).  Fixed-length
 * records (pire_hip_run_pair_strided; len >= 256 with an EVEN number of whole 128-byte tiles, i.e. (len / 128) % 2 == 0
 * -- 256..383, 512..639, ... --, stride a multiple of 16, text 16-byte aligned, at least 64 records) take ONE pass with
 * both tables' dense rows in LDS: the text is read once and the two lookups of a byte overlap; what is left of a record
 * behind its whole tiles (len % 128 bytes) is walked byte by byte in the same pass.  Anything else, and the last
 * n mod 64 records, takes two ordinary passes behind the same call.  Any output pointer may be NULL.
 */
int pire_hip_run_pair(pire_hip_table* t1, pire_hip_table* t2, const void* text, const uint64_t* offsets, uint64_t n,
                      uint32_t flags, uint32_t* out_state_idx1, uint32_t* out_state_idx2, uint8_t* out_final, void* stream);
int pire_hip_run_pair_strided(pire_hip_table* t1, pire_hip_table* t2, const void* text, uint64_t n, uint64_t len,
                              uint64_t stride, uint32_t flags, uint32_t* out_state_idx1, uint32_t* out_state_idx2,
                              uint8_t* out_final, void* stream);

/*
 * Pire::LongestSuffix / Pire::ShortestSuffix (run.h:313-362) for n strings: every string is walked BACKWARDS from its
 * last byte (the scanner is normally compiled from Fsm::Reverse(), pire_ut.cpp:283).  out_len[i] = length of the
 * longest (shortest) suffix accepted -- the reference returns the pointer (last byte) - out_len[i] -- or -1 where the
 * reference returns a null pointer.  through_end / through_begin as the reference's throughEndMark / throughBeginMark
 * (in that order: the walk starts at the end).  Scanning stops at the first dead state.  flags: PIRE_HIP_RUN_ON_DEVICE.
 * Pinned by tests/pire_ut.cpp:278-306 (PrefixSuffix) and 470-471 (ScanBoundaries on reversed texts).
 */
int pire_hip_suffix(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, int longest,
                    int through_end, int through_begin, uint32_t flags, int64_t* out_len, void* stream);

/* Name of the kernel the last run on this thread dispatched to ("tiled", "ragged", "generic", "ragged_prefix",
 * "prefix", "suffix", "pair_tiled", "ragged_half_final", "half_final", "segmented", "segmented+plain"); diagnostics. */
const char* pire_hip_last_kernel(void);
/* ",name,name,...": the kernels (names as pire_hip_last_kernel reports them) that have passed a first-use self-test in this
 * process so far (pire_hip_config.selftest); thread-local copy.  Diagnostics: tests/test_selftest.py holds every name the
 * library can emit against it. */
const char* pire_hip_selftested_kernels(void);
/* The instantiation behind it where there are several (e.g. "pirehip::ScanTiledKernel<16,2,nt,5>" for "tiled");
 * otherwise the same string as pire_hip_last_kernel(). */
const char* pire_hip_last_kernel_symbol(void);

/* Milliseconds the most recent kernel launched by this thread took, measured with hipEvents on the
 * launch stream when timing was enabled with pire_hip_set_timing(1).  Synchronises the stream. */
int   pire_hip_set_timing(int enabled);
float pire_hip_last_kernel_ms(void);

/* ---- SlowScanner (BASELINE config 5b) --------------------------------------------------------------- */
/*
 * Pire::SlowScanner (pire/scanners/slow.h:51-420): NFA simulation for patterns whose DFA would not fit anywhere
 * (e.g. /x.{40}$/).  Its state is the SET of active NFA states (slow.h:63-74), so results are the Final flag
 * (slow.h:152-158) and, optionally, the set itself as a bitset.  Ingests SlowScanner::Save() bytes
 * (pire/scanner_io.cpp:71-111).  Up to 256 NFA states the set of a string lives in the registers of ONE lane
 * (one string per lane); larger automata -- the reference has no limit, easy.h:155-161 falls back to this scanner
 * exactly when determinisation blows up -- keep the reference's sparse jump lists and give every string a whole wave
 * (the set is a bitset in LDS, or in device memory when 2 * states / 8 bytes do not fit there).
 */
typedef struct pire_hip_slow_table pire_hip_slow_table;

typedef struct pire_hip_slow_info {
	uint32_t states;      /* SlowScanner::Size()            slow.h:83-84 */
	uint32_t letters;     /* SlowScanner::GetLettersCount() slow.h:81    */
	uint32_t start;       /* m.start                        slow.h:343   */
	uint32_t words;       /* (states + 31) / 32: uint32 words of one state set */
	uint32_t empty;       /* SlowScanner::Empty()           slow.h:85    */
	uint32_t reserved;
	uint64_t mask_bytes;  /* size of the (state, letter) -> target-set matrix */
} pire_hip_slow_info;

int pire_hip_slow_table_create(const void* save_blob, size_t len, pire_hip_slow_table** out);
void pire_hip_slow_table_destroy(pire_hip_slow_table* t);
int pire_hip_slow_table_get_info(const pire_hip_slow_table* t, pire_hip_slow_info* out);
/* What a run of n strings would launch (performance only; every form gives the same results), under the current
 * configuration: `ragged` != 0 for the offsets form, 0 for fixed-length records; `cus` = compute units to plan for, 0 = those
 * of the current device (any other value needs no device).  out[0] = the kernel that runs first (0 the 16-slot list kernel,
 * 1 the bitset kernel, 2 the wave-per-string kernel), out[1] = the kernel that walks whole strings (1 or 2: after the list
 * kernel it takes the strings that left it), out[2] = words per lane of the bitset kernel (1, 2, 4, 8; 0: more than 256
 * states), out[3] = 1 if the table has a list form, out[4] / out[5] = 1 if the bitset kernel keeps its first-targets table /
 * its masks in LDS, out[6..9] = threads per block, blocks, LDS bytes and grid-stride passes of the first kernel,
 * out[10] = waves per block of the wave-per-string kernel, out[11] / out[12] / out[13] = 1 if that kernel keeps the jump
 * positions / the jumps / the state sets in LDS, out[14] = 1 if the list kernel takes the strings by length class,
 * out[15..18] = as out[6..9] for the kernel of out[1], out[19] = the compute units planned for, out[20..23] = 0. */
int pire_hip_slow_table_plan(const pire_hip_slow_table* t, uint64_t n, uint32_t ragged, uint32_t cus, uint32_t out[24]);

/*
 * For each string: Initialize (slow.h:89-95); Begin() if flags&BEGIN; Run (the SlowScanner specialisation,
 * slow.h:436-451); End() if flags&END.  out_final[i] = Final(state).  out_state_bits (nullable): `words` uint32 per
 * string, bit s set <=> NFA state s is in the final state set.  out_counts (nullable) uint64[2] accumulated:
 * [0] += strings ending Final, [1] += n.  Pointer/flag conventions as pire_hip_run.
 */
int pire_hip_slow_run(pire_hip_slow_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                      uint8_t* out_final, uint32_t* out_state_bits, uint64_t* out_counts, void* stream);
int pire_hip_slow_run_strided(pire_hip_slow_table* t, const void* text, uint64_t n, uint64_t len, uint64_t stride,
                              uint32_t flags, uint8_t* out_final, uint32_t* out_state_bits, uint64_t* out_counts,
                              void* stream);

/*
 * From Final flags to the strings that matched -- or did not: a compacted, ascending list of their indices.  It takes no
 * table and no text: it reads one flag byte per string, what pire_hip_slow_run wrote (out_final), and a flag counts as set
 * when it is not 0 -- so the pass also works behind out_final of pire_hip_run and pire_hip_run_pair.
 *   selected(i) <=> (final[i] != 0) != (mode == PIRE_HIP_FINAL_SELECT_ZERO)
 * mode: 0 selects the strings whose flag is set, PIRE_HIP_FINAL_SELECT_ZERO those whose flag is not (grep -v).
 * out_hits[hit_cap] (nullable), hit_cap, *out_hit_count (required): exactly pire_hip_select's -- ascending, the full count
 * also when it exceeds hit_cap, only the first min(count, hit_cap) entries written and nothing behind them; n == 0 writes
 * a count of 0.  n < 2^32.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> every pointer is a device pointer and the call only enqueues on `stream`: classify per
 *        tile of 1 024 strings, the one-block scan of pire_hip_select, scatter; no atomics, no block waits for another: the
 *        same input gives the same bits.  Scratch (n / 8 + n / 256 bytes) comes from the stream-ordered allocator: the rule
 *        and the capture-mode caveat stated at pire_hip_select.  `final` may have any alignment.  Otherwise host pointers:
 *        staged, synchronises, the list comes back only as far as it was written.
 * PIRE_HIP_EINVAL before any device is touched: a mode other than the two; null out_hit_count; n > 0 with null final;
 * hit_cap > 0 with null out_hits; n >= 2^32.
 * pire_hip_last_kernel() is not changed by the pass.  No first-use self-test (it takes no table, as pire_hip_split).
 */
#define PIRE_HIP_FINAL_SELECT_ZERO 1u   /* `mode` */
int pire_hip_final_select(const uint8_t* final, uint64_t n, uint32_t mode, uint32_t flags, uint64_t* out_hits, uint64_t hit_cap,
                          uint64_t* out_hit_count, void* stream);

/*
 * pire_hip_slow_run[_strided] followed by pire_hip_final_select on the same stream, behind whichever launch form the scan
 * takes (list kernel, bitset kernel, wave-per-string kernel, list then hand-on).  t .. flags, out_final, out_state_bits,
 * out_counts: as the run call; out_final is nullable here: the flags then live in stream-ordered scratch of the library's
 * own.  mode, out_hits, hit_cap, out_hit_count: as pire_hip_final_select.  With host pointers the text is staged once, and
 * scan and pass run on the staged copy before anything comes back.  Hit indices are relative to the whole batch.  They
 * refuse what the run call refuses and what pire_hip_final_select refuses.  pire_hip_last_kernel() names the scan's kernel.
 */
int pire_hip_slow_run_select(pire_hip_slow_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                             uint32_t mode, uint8_t* out_final, uint32_t* out_state_bits, uint64_t* out_counts,
                             uint64_t* out_hits, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);
int pire_hip_slow_run_select_strided(pire_hip_slow_table* t, const void* text, uint64_t n, uint64_t len, uint64_t stride,
                                     uint32_t flags, uint32_t mode, uint8_t* out_final, uint32_t* out_state_bits,
                                     uint64_t* out_counts, uint64_t* out_hits, uint64_t hit_cap, uint64_t* out_hit_count,
                                     void* stream);

/*
 * Raw bytes in, the lines a SlowScanner matches -- or, with mode = PIRE_HIP_FINAL_SELECT_ZERO, does not match -- out: the
 * split into scratch, the slow scan on the lines with the flags in scratch, the pass.  out_line_count (required), delim,
 * out_hits (the numbers of the lines), out_hit_spans[hit_cap][2] (nullable, needs out_hits: the whole line of hit k as a
 * byte range of raw, delimiter not included), hit_cap, out_hit_count, flags (BEGIN | END | ON_DEVICE), the one
 * synchronisation of `stream` (reading n back; the call adds none) and the refusal of 2^32 lines: as
 * pire_hip_run_lines_select, which has `want` and masks where this has `mode`.  pire_hip_slow_lines_gather adds the gather
 * of the selected lines from raw: tail, out_hits (nullable: the library keeps the hit list to itself), out_text, text_cap,
 * out_offsets (hit_cap + 1 entries), out_bytes as pire_hip_run_lines_gather.  With mode = PIRE_HIP_FINAL_SELECT_ZERO and
 * tail = delim the bytes in out_text are what `grep -v` prints for the buffer.  Host pointers with size == 0: zeros, no
 * device is touched.  PIRE_HIP_EINVAL before any device is touched: null table, what pire_hip_final_select refuses (in the
 * gather form hit_cap > 0 with null out_hits excepted), out_hit_spans without out_hits, delim > 255, null out_line_count,
 * size > 0 with null raw, and what pire_hip_gather refuses of its outputs.  pire_hip_last_kernel() names the scan's kernel.
 */
int pire_hip_slow_lines_select(pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                               uint32_t mode, uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans,
                               uint64_t hit_cap, uint64_t* out_hit_count, void* stream);
int pire_hip_slow_lines_gather(pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                               uint32_t mode, uint32_t tail, uint64_t* out_line_count, uint64_t* out_hits, uint64_t hit_cap,
                               uint64_t* out_hit_count, void* out_text, uint64_t text_cap, uint64_t* out_offsets,
                               uint64_t* out_bytes, void* stream);

/* ---- one process, several GPUs (BASELINE config C4) --------------------------- */
/*
 * The path shards by string: a string's walk depends on nothing but the table and its own bytes (run.h:271-275),
 * so GPU g scans its contiguous range of strings with no data-path exchange; the only collective is the sum of the
 * uint64[regexps+2] match counters -- one all-reduce over RCCL (xGMI) per batch, latency bound (80 bytes for 8
 * regexps).  The reference has no counterpart (a single-threaded CPU library); this is the C-ABI form of what
 * bench.py does with one process per GPU.  One table handle serves every device (it keeps an image per device).
 * RCCL is loaded at run time; without it (or when the communicator cannot be built) the per-device counters are
 * summed on the host -- pire_hip_multi_reduce_backend() says which ("rccl" or "host (...reason)").
 */
typedef struct pire_hip_multi pire_hip_multi;

/* One shard: fixed-length records resident on ITS device (pointers are device pointers of that device). */
typedef struct pire_hip_shard {
	const void*     text;
	uint64_t        n, len, stride;
	const uint32_t* init_state_idx;   /* nullable */
	uint32_t*       out_state_idx;    /* nullable */
	uint8_t*        out_final;        /* nullable */
} pire_hip_shard;

/* devices == NULL: HIP devices 0 .. ndev-1 (ndev <= 0: all of them).  Creates one stream and one counter buffer per
 * device and, for two or more distinct devices, the RCCL communicator (ncclCommInitAll). */
int  pire_hip_multi_create(const int* devices, int ndev, pire_hip_multi** out);
void pire_hip_multi_destroy(pire_hip_multi* m);
int  pire_hip_multi_device_count(const pire_hip_multi* m);
const char* pire_hip_multi_reduce_backend(const pire_hip_multi* m);

/*
 * Scan shards[g] on device g of `m` (all devices run concurrently, each on its own stream), then reduce the match
 * counters: out_counts (host memory, uint64[regexps+2], nullable) RECEIVES the totals over all shards (it is not
 * accumulated into).  flags: PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END | PIRE_HIP_RUN_GENERIC.  Returns when every
 * device has finished.  The caller's current device is restored.
 */
int pire_hip_multi_run_strided(pire_hip_multi* m, pire_hip_table* t, const pire_hip_shard* shards, uint32_t flags,
                               uint64_t* out_counts);
/*
 * Convenience form for a batch in HOST memory: strings [lo_g, hi_g) -- contiguous, balanced ranges -- are copied to
 * device g, scanned, and the per-string results copied back into the caller's arrays (PCIe-inclusive, like the
 * host-pointer mode of pire_hip_run).
 */
int pire_hip_multi_run_strided_host(pire_hip_multi* m, pire_hip_table* t, const void* text, uint64_t n, uint64_t len,
                                    uint64_t stride, uint32_t flags, const uint32_t* init_state_idx,
                                    uint32_t* out_state_idx, uint8_t* out_final, uint64_t* out_counts);

/* One shard of an OFFSET batch (what the reference's callers have: ragged lines, samples/pigrep/pigrep.cpp:38-45):
 * text and n + 1 byte offsets resident on ITS device, string i = text[offsets[i], offsets[i+1]). */
typedef struct pire_hip_shard_offsets {
	const void*     text;
	const uint64_t* offsets;
	uint64_t        n;
	const uint32_t* init_state_idx;   /* nullable */
	uint32_t*       out_state_idx;    /* nullable */
	uint8_t*        out_final;        /* nullable */
} pire_hip_shard_offsets;

/* pire_hip_multi_run_strided for offset batches: shards[g] lives on device g of the runner, all devices scan
 * concurrently (pire_hip_run on the runner's stream of each device), the counters are reduced as above. */
int pire_hip_multi_run(pire_hip_multi* m, pire_hip_table* t, const pire_hip_shard_offsets* shards, uint32_t flags,
                       uint64_t* out_counts);

/* Host-resident offset batch: cut into one contiguous run of whole strings per device, balanced by BYTES (a shard
 * boundary is the string boundary nearest to g / G of the text: ragged strings make string counts a poor measure of
 * work), staged through per-device buffers the runner keeps between calls (no allocation per call once they have
 * grown), scanned concurrently, results written back in string order.  offsets[0] need not be 0. */
int pire_hip_multi_run_host(pire_hip_multi* m, pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n,
                            uint32_t flags, const uint32_t* init_state_idx, uint32_t* out_state_idx, uint8_t* out_final,
                            uint64_t* out_counts);

/* First string of every shard the last pire_hip_multi_run_host / _run_strided_host call made: out[0 .. devices], the
 * last entry = n.  Diagnostics (tests, the per-device rates of a benchmark). */
int pire_hip_multi_last_split(const pire_hip_multi* m, uint64_t* out, int capacity);

/* ---- memory helpers ------------------------------------------------------------------------------- */
/*
 * Thin wrappers over the HIP runtime so that a caller of this ABI (and the header-only C++ shim) need not link HIP
 * itself.  Text placed in pire_hip_host_alloc() memory is pinned: the host-pointer mode of pire_hip_run then moves it
 * by plain DMA, overlapped chunk by chunk with the scan (pageable text is staged by the runtime; both are measured in
 * DESIGN.md).  Copies are asynchronous on `stream` (NULL = default stream); synchronise before reading the result.
 */
int  pire_hip_host_alloc(size_t bytes, void** out);
void pire_hip_host_free(void* p);
int  pire_hip_device_alloc(size_t bytes, void** out);
void pire_hip_device_free(void* p);
int  pire_hip_copy_to_device(void* dst_device, const void* src_host, size_t bytes, void* stream);
int  pire_hip_copy_to_host(void* dst_host, const void* src_device, size_t bytes, void* stream);
int  pire_hip_memset_device(void* dst_device, int value, size_t bytes, void* stream);
int  pire_hip_stream_synchronize(void* stream);

/* ---- errors ---------------------------------------------------------------------------------------- */
const char* pire_hip_last_error(void);
int pire_hip_device_count(void);

/* ---- benchmark utility (not part of the reference surface) ------------------------------------------ */
/* Witnesses planted into the synthetic corpus: string s carries plant (s mod (nplants+1)) - 1, none when that is
 * -1; at_tail: at the end of the string (for '$'-anchored patterns), otherwise at a generated offset. */
#define PIRE_HIP_CORPUS_MAX_PLANTS 16
#define PIRE_HIP_CORPUS_PLANT_BYTES 64
typedef struct pire_hip_corpus_plants {
	uint32_t nplants;
	uint32_t len[PIRE_HIP_CORPUS_MAX_PLANTS];
	uint32_t at_tail[PIRE_HIP_CORPUS_MAX_PLANTS];
	uint8_t  bytes[PIRE_HIP_CORPUS_MAX_PLANTS][PIRE_HIP_CORPUS_PLANT_BYTES];
} pire_hip_corpus_plants;

/*
 * Fill device memory with the synthetic corpus of SURVEY.md section 8d: string s occupies
 * out[(s-first)*stride, +len).  `plants` is a host pointer to a pire_hip_corpus_plants (the layout of
 * oracle/corpus.h, the generator's CPU twin) or NULL.  Bit-identical with oracle/corpus.c for the same (seed, s).
 */
int pire_hip_corpus_fill(void* device_out, uint64_t seed, uint64_t first, uint64_t count, uint64_t len,
                         uint64_t stride, const void* plants, void* stream);

/* ---- Pire::CountingScanner / Pire::AdvancedCountingScanner (extra/count.h) ------------------------- */

/*
 * The counting scanners of pire/extra/count.h: "count the occurrences of `re` separated by `sep`", up to 16 regexps
 * glued into one scanner.  They are LoadedScanner tables (scanners/loaded.h: transitions carry an Action) whose
 * TakeAction keeps a current and a total counter per regexp in the state (count.h:119-234).  Both classes serialise
 * through LoadedScanner::Save (scanner_io.cpp:172-189) with the same header, so the caller says which TakeAction
 * the table was built for: PIRE_HIP_COUNTING_BASIC = CountingScanner (increment, then reset; count.h:251-257),
 * PIRE_HIP_COUNTING_ADVANCED = AdvancedCountingScanner (reset, then increment; count.h:287-295).
 * PIRE_HIP_COUNTING_NOGLUELIMIT = NoGlueLimitCountingScanner, whose blob also carries the action lists.
 * Pinned by tests/count_ut.cpp:95-200.
 */
typedef struct pire_hip_counting_table pire_hip_counting_table;

#define PIRE_HIP_COUNTING_BASIC 0
#define PIRE_HIP_COUNTING_ADVANCED 1
#define PIRE_HIP_COUNTING_NOGLUELIMIT 2   /* NoGlueLimitCountingScanner: its own Save() form (count.cpp:1009-1018), any
                                            number of regexps; resets before increments (count.h:404-437) */

typedef struct pire_hip_counting_info {
	uint32_t states;    /* Size(), loaded.h:112 */
	uint32_t letters;   /* LettersCount(), loaded.h:118 */
	uint32_t regexps;   /* RegexpsCount(), loaded.h:116 */
	uint32_t initial;   /* StateIndex(Initialize()), count.h:127-133, 171 */
} pire_hip_counting_info;

int pire_hip_counting_table_create(const void* save_blob, size_t len, pire_hip_counting_table** out);
void pire_hip_counting_table_destroy(pire_hip_counting_table* t);
int pire_hip_counting_table_get_info(const pire_hip_counting_table* t, pire_hip_counting_info* out);
/* Which device forms the table has (performance only; every form gives the same results): out[0] = counter registers of
 * the 16-bit-entry form (0: none), out[1] = its LDS bytes; out[2] = 1 if the byte-indexed row form applies (<= 64 states),
 * out[3] = its LDS bytes; out[4] = counter registers of the letter-indexed row form (0: none), out[5] = its LDS bytes,
 * out[6] = its distinct actions; out[7] = 0. */
int pire_hip_counting_table_forms(const pire_hip_counting_table* t, uint32_t out[8]);

/*
 * Per string i: Initialize; Begin() if flags & BEGIN; Run; End() if flags & END (tests/count_ut.cpp:54-63), then
 *   out_results[i * regexps + r] = State::Result(r) = max(current[r], total[r])   (count.h:206)
 *   out_state_idx[i] (nullable)  = StateIndex of the end state                     (count.h:171)
 * flags: PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END | PIRE_HIP_RUN_ON_DEVICE.
 */
int pire_hip_counting_run(pire_hip_counting_table* t, int kind, const void* text, const uint64_t* offsets, uint64_t n,
                          uint32_t flags, uint32_t* out_state_idx, uint32_t* out_results, void* stream);

/* ---- Pire::CapturingScanner (extra/capture.h) ------------------------------------------------------ */

/*
 * The capturing scanner of pire/extra/capture.h:49-162: one regexp, the substring matched by ONE pair of parentheses
 * (built with Features::Capture(i), extra/capture.cpp).  It is a LoadedScanner table too (create it with
 * pire_hip_counting_table_create): transitions carry BeginCapture = 1 / EndCapture = 2, TakeAction records the step
 * counter (capture.h:96-116), Final comes from the state tags (capture.h:134).  Per string i, after
 * Initialize; Begin(); Run(); End() (tests/capture_ut.cpp:75-83):
 *   out_begin[i], out_end[i] = State::Begin(), State::End(): 1-based byte positions (the BeginMark step is counted;
 *                              the captured text is [begin - 1, end - 1), capture_ut.cpp:85-91), -1 where unset;
 *                              State::Captured() == (out_begin[i] >= 0 && out_end[i] >= 0)
 *   out_final[i], out_state_idx[i] (nullable) = Final / StateIndex of the end state.
 */
int pire_hip_capture_run(pire_hip_counting_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                         uint32_t* out_state_idx, uint8_t* out_final, int64_t* out_begin, int64_t* out_end, void* stream);

/* ---- the captured substrings, on the device ------------------------------------------------------------------- */

/*
 * From capture positions to byte ranges: the strings that captured, as a compacted, ascending list, and where their
 * captured text lies -- the input of pire_hip_gather_spans.  It takes no table and no text: it reads what
 * pire_hip_capture_run wrote (begin, end, final of the same n strings, offsets[n + 1]), behind any of the capture kernels.
 *   B           = (flags & PIRE_HIP_RUN_BEGIN) ? 1 : 0          the BeginMark step is counted (capture.h:96-116)
 *   len_i       = offsets[i + 1] - offsets[i]
 *   captured(i) = begin[i] >= 0 && end[i] >= 0                    State::Captured(), capture.h:61
 *   selected(i) = captured(i) && (!need_final || final[i] != 0)
 *   b_i         = clamp(begin[i] - B, 0, len_i)
 *   e_i         = clamp(end[i]   - B, b_i, len_i)
 *   span(i)     = [offsets[i] + b_i, offsets[i] + e_i)            a byte range of `text`
 * out_hits[hit_cap] (nullable): the indices of the selected strings, ascending.  out_spans[hit_cap][2] (nullable, and it
 * does not need out_hits): their spans.  *out_hit_count (required): the number of selected strings, also when it exceeds
 * hit_cap; only the first min(count, hit_cap) entries are written, nothing behind them.  n == 0 writes a count of 0.
 * n < 2^32.
 * The clamp: for a well-formed capture the span is exactly the reference's [str + Begin() - 1, str + End() - 1)
 * (capture_ut.cpp:85-91), [str + Begin(), str + End()) for a runner that never called Begin().  That helper is undefined
 * where an action fires on the BeginMark step (begin == 0 under Begin()) and where end < begin; a device pass must not
 * be.  Such a string is still captured, as the reference says: it stays in the list, its range clamped into the string,
 * possibly empty.  So a span never leaves [offsets[i], offsets[i + 1]], whatever int64 the ON_DEVICE form is given.
 * flags: PIRE_HIP_RUN_BEGIN -> the flag the capture call was made with.  PIRE_HIP_RUN_ON_DEVICE -> every pointer is a
 *        device pointer and the call only enqueues on `stream`: three kernels (classify per tile of 1 024 strings, the
 *        one-block scan of pire_hip_select, scatter), no atomics -- the same input gives the same bits.  Scratch
 *        (n / 8 + n / 256 bytes) comes from the stream-ordered allocator: the rule and the capture-mode caveat stated at
 *        pire_hip_select.  Otherwise host pointers: staged, synchronises.
 * PIRE_HIP_EINVAL before any device is touched: null out_hit_count; n > 0 with null offsets, begin or end; need_final
 * with null final; hit_cap > 0 with null out_hits and null out_spans; n >= 2^32.
 * pire_hip_last_kernel() is not changed by the pass.  No first-use self-test (as pire_hip_select).
 */
int pire_hip_capture_select(const uint64_t* offsets, uint64_t n, uint32_t flags,
                            const int64_t* begin, const int64_t* end, const uint8_t* final, int need_final,
                            uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);

/*
 * pire_hip_capture_run followed by pire_hip_capture_select on the same stream.  t .. flags (BEGIN / END / ON_DEVICE /
 * GENERIC): as pire_hip_capture_run; the pass gets flags & PIRE_HIP_RUN_BEGIN.  out_state_idx, out_final, out_begin and
 * out_end are all nullable here: what the pass needs and the caller has no array for lives in stream-ordered scratch of
 * the library's own.  With host pointers the text is staged once, and scan and pass run on the staged copy before
 * anything comes back.  It refuses what pire_hip_capture_run refuses (the null position arrays excepted) and what
 * pire_hip_capture_select refuses.  pire_hip_last_kernel() names the capture kernel.
 */
int pire_hip_capture_run_select(pire_hip_counting_table* t, const void* text, const uint64_t* offsets, uint64_t n,
                                uint32_t flags, int need_final,
                                uint32_t* out_state_idx, uint8_t* out_final, int64_t* out_begin, int64_t* out_end,
                                uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap, uint64_t* out_hit_count,
                                void* stream);

/*
 * Raw bytes in, the captured field of every line that captured out: pire_hip_run_lines_gather for a capturing scanner
 * (`grep -o` with one pair of parentheses).  The split into scratch, the capture scan on the lines, the pass -- its
 * spans counted in raw: line i of the split buffer lies i bytes further into raw --, the gather from raw through them.
 * out_line_count, delim, the one synchronisation of `stream` and the refusal of 2^32 lines (PIRE_HIP_EUNSUPPORTED): as
 * pire_hip_run_lines_select.  out_hits (nullable): the numbers of the lines that captured; out_spans (nullable): byte
 * ranges of raw; need_final, hit_cap, out_hit_count: as pire_hip_capture_select.  tail, out_text, text_cap, out_offsets
 * (hit_cap + 1 entries), out_bytes: as pire_hip_gather_spans.  All four gather outputs null (text_cap == 0): spans only,
 * the gather is skipped; any other combination of nulls is what pire_hip_gather refuses.  Host pointers with size == 0:
 * zeros (out_offsets[0] = 0 where it is not null), no device is touched.  It also refuses delim > 255, null
 * out_line_count, size > 0 with null raw, out_text overlapping raw, and what pire_hip_capture_select refuses.
 */
int pire_hip_capture_lines_gather(pire_hip_counting_table* t, const void* raw, uint64_t size, uint32_t delim,
                                  uint32_t flags, int need_final, uint32_t tail,
                                  uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_spans,
                                  uint64_t hit_cap, uint64_t* out_hit_count,
                                  void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes,
                                  void* stream);

/* ---- SlowCapturingScanner: exact and non-greedy captures ----------------------------------------------------------- */
/*
 * Pire::SlowCapturingScanner (pire/extra/capture.h:170-581): the NFA walk with priorities, the one scanner of the reference
 * that tells .*?(re) from .*(re) and (A)|A from A|(A) -- the DFA behind pire_hip_capture_run records the first BeginCapture
 * and EndCapture it meets.  Ingests SlowScanner::Save() bytes WITH the action area (scanner_io.cpp:71-110); the blob does not
 * say whether it has one, so a blob that ends where a plain SlowScanner's does is PIRE_HIP_EFORMAT.  Header checks as
 * pire_hip_slow_table_create.  Up to 1 024 states; a larger scanner is PIRE_HIP_EUNSUPPORTED at create.  An empty scanner
 * loads, as it does there: one state with nowhere to go -- no string matches or captures.
 * The table holds the flat form of the reference's walk, built on the host at create in O(states^2 *
 * letters): for every (state, letter) the ordered list NextAndGetToGroups leaves, per state whether it matches at the end of
 * the string, and what Initialize() leaves.  The library has no host walk: pire_hip_slow_capture_table_image exports that
 * form, as pire_hip_table_layout does for the fast scanner's.
 */
typedef struct pire_hip_slow_capture_table pire_hip_slow_capture_table;

typedef struct pire_hip_slow_capture_info {
	uint32_t states;        /* SlowScanner::Size() */
	uint32_t letters;       /* SlowScanner::GetLettersCount() */
	uint32_t start;         /* m.start */
	uint32_t entries;       /* of all lists together */
	uint32_t longest_list;  /* entries of the longest list(state, letter) */
	uint32_t init_len;      /* states Initialize() leaves on the list */
	uint32_t init_matched;  /* 1 if Initialize() leaves a match */
	uint32_t empty;         /* SlowScanner::Empty() */
	uint32_t reserved[4];
} pire_hip_slow_capture_info;

int pire_hip_slow_capture_table_create(const void* save_blob, size_t len, pire_hip_slow_capture_table** out);
void pire_hip_slow_capture_table_destroy(pire_hip_slow_capture_table* t);
int pire_hip_slow_capture_table_get_info(const pire_hip_slow_capture_table* t, pire_hip_slow_capture_info* out);
/*
 * The table's image.  list_pos[states * letters + 1]: list(s, l) is entries[list_pos[s * letters + l] .. list_pos[s * letters
 * + l + 1]).  entries[entries_cap] (entries_cap >= info.entries): bits 0-15 the target state, bit 16 the path from s to it
 * carries a BeginCapture, bit 17 an EndCapture; the targets of one list are distinct.  state_flags[states]: bit 0 the state
 * matches at the end of the string (Captured()'s `matched`), bit 1 Captured()'s return for that state without a begin.
 * init[init_len][3]: (state, begin, end) of Initialize()'s list, positions 0 or -1 (not set); init_match[3]: the match it
 * leaves where info.init_matched.  letters[260]: the letter of every Char (256 bytes, then Epsilon = 257, BeginMark = 258,
 * EndMark = 259).  A step on a byte and GetCapture() over these arrays: DESIGN.md 4.23, restated in tests/test_slow_capture.py.
 */
int pire_hip_slow_capture_table_image(const pire_hip_slow_capture_table* t, uint32_t* list_pos, uint32_t* entries,
                                      uint64_t entries_cap, uint8_t* state_flags, int64_t* init, int64_t* init_match,
                                      uint8_t* letters);

/*
 * For each string: Initialize, Run, GetCapture (capture_ut.cpp:77-83, 259-272) -- the scanner takes the begin and end marks
 * itself.  out_captured[i] = GetCapture()'s return.  out_begin[i] / out_end[i] = final.GetBegin() / GetEnd() where GetCapture
 * assigned `final`, -1 for npos and where it assigned nothing: 0-based byte offsets into the string, the captured text is
 * [begin, end).  out_matched (nullable): 1 where `final` was assigned (the string matched, captured or not).
 * flags: PIRE_HIP_RUN_ON_DEVICE as pire_hip_slow_run (device pointers, the call only enqueues); every other flag but BEGIN /
 * END is ignored, as there.  One wave per string: the ordered state list (state, begin, end) lives in LDS, 24 bytes per
 * state and wave; the image stays in LDS up to 48 KB and in device memory beyond.
 * PIRE_HIP_EINVAL before any device is touched: null table; PIRE_HIP_RUN_BEGIN or PIRE_HIP_RUN_END; n > 0 with null offsets,
 * out_captured, out_begin or out_end; with host pointers what pire_hip_run refuses of a batch, and a string of 2^32 - 1 bytes
 * or more (positions are 32 bits wide on the device; with ON_DEVICE this is the caller's precondition).  n == 0 and empty
 * strings are legal.  pire_hip_last_kernel() names "slow_capture".  No first-use self-test, as pire_hip_slow_run.
 */
int pire_hip_slow_capture_run(pire_hip_slow_capture_table* t, const void* text, const uint64_t* offsets, uint64_t n,
                              uint32_t flags, uint8_t* out_captured, int64_t* out_begin, int64_t* out_end,
                              uint8_t* out_matched, void* stream);

/*
 * pire_hip_slow_capture_run followed by pire_hip_capture_select on the same stream: the pass gets no PIRE_HIP_RUN_BEGIN,
 * final = the captured flags and need_final = 1, so hit k is a string that captured and its span is [offsets[i] + begin,
 * offsets[i] + end), clamped as that pass clamps.  out_captured, out_begin, out_end and out_matched are all nullable here:
 * what the pass needs and the caller has no array for lives in stream-ordered scratch.  out_hits, out_spans, hit_cap,
 * out_hit_count: as pire_hip_capture_select.  It refuses what the run call refuses (the null result arrays excepted) and
 * what pire_hip_capture_select refuses.
 */
int pire_hip_slow_capture_run_select(pire_hip_slow_capture_table* t, const void* text, const uint64_t* offsets, uint64_t n,
                                     uint32_t flags, uint8_t* out_captured, int64_t* out_begin, int64_t* out_end,
                                     uint8_t* out_matched, uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap,
                                     uint64_t* out_hit_count, void* stream);

/*
 * Raw bytes in, the captured field of every line that captured out -- `grep -o` with lazy quantifiers.  Arguments, nulls,
 * refusals and the one synchronisation of `stream` as pire_hip_capture_lines_gather, which has need_final where this has
 * none (a line is listed when GetCapture() returned true); flags: PIRE_HIP_RUN_ON_DEVICE only, BEGIN / END are refused.
 */
int pire_hip_slow_capture_lines_gather(pire_hip_slow_capture_table* t, const void* raw, uint64_t size, uint32_t delim,
                                       uint32_t flags, uint32_t tail, uint64_t* out_line_count, uint64_t* out_hits,
                                       uint64_t* out_spans, uint64_t hit_cap, uint64_t* out_hit_count, void* out_text,
                                       uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* stream);

/* ---- the matched heads and tails, on the device ------------------------------------------------------------------ */

#define PIRE_HIP_AFFIX_HEAD 0u   /* the matched prefix */
#define PIRE_HIP_AFFIX_TAIL 1u   /* the matched suffix */
#define PIRE_HIP_AFFIX_REST 2u   /* what the head and the tail leave */

/*
 * From prefix and suffix lengths to byte ranges: the strings that matched, as a compacted, ascending list, and where the
 * matched head, the matched tail, or what lies between them is -- the input of pire_hip_gather_spans.  It takes no table
 * and no text: it reads what pire_hip_prefix and pire_hip_suffix wrote for the same n strings (head_len, tail_len; either
 * may be null, not both), plus offsets[n + 1].
 *   len_i       = offsets[i+1] >= offsets[i] ? offsets[i+1] - offsets[i] : 0
 *   selected(i) = (head_len == NULL || head_len[i] >= 0) && (tail_len == NULL || tail_len[i] >= 0)
 *   h_i         = head_len ? min(head_len[i], len_i)       : 0
 *   t_i         = tail_len ? min(tail_len[i], len_i)       : 0
 *   r_i         = tail_len ? min(tail_len[i], len_i - h_i) : 0     (REST: the tail gives way to the head where they overlap)
 *   HEAD: [offsets[i],              offsets[i] + h_i)              needs head_len
 *   TAIL: [offsets[i] + len_i - t_i, offsets[i] + len_i)           needs tail_len
 *   REST: [offsets[i] + h_i,         offsets[i] + len_i - r_i)     needs at least one of them
 * A length of 0 is a match -- the scanner accepts the empty prefix --: the string is selected and its span is empty.  A
 * length of -1 is the reference's null pointer: the string is not selected.  A span never leaves
 * [offsets[i], offsets[i + 1]], whatever int64 the ON_DEVICE form is given (as pire_hip_capture_select, for the same reason).
 * out_hits[hit_cap] (nullable): the indices of the selected strings, ascending.  out_spans[hit_cap][2] (nullable, and it
 * does not need out_hits): their spans.  *out_hit_count (required): the number of selected strings, also when it exceeds
 * hit_cap; only the first min(count, hit_cap) entries are written, nothing behind them.  n == 0 writes a count of 0.
 * n < 2^32.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> every pointer is a device pointer and the call only enqueues on `stream`: three kernels
 *        (classify per tile of 1 024 strings, the one-block scan of pire_hip_select, scatter), no atomics -- the same input
 *        gives the same bits.  Scratch (n / 8 + n / 256 bytes) comes from the stream-ordered allocator: the rule and the
 *        capture-mode caveat stated at pire_hip_select.  Otherwise host pointers: staged, synchronises.
 * PIRE_HIP_EINVAL before any device is touched: unknown part; n > 0 with null head_len and null tail_len; HEAD without
 * head_len, TAIL without tail_len; n > 0 with null offsets; null out_hit_count; hit_cap > 0 with null out_hits and null
 * out_spans; n >= 2^32.
 * pire_hip_last_kernel() is not changed by the pass.  No first-use self-test (as pire_hip_select).
 */
int pire_hip_affix_select(const uint64_t* offsets, uint64_t n, uint32_t part, uint32_t flags,
                          const int64_t* head_len, const int64_t* tail_len,
                          uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap,
                          uint64_t* out_hit_count, void* stream);

#define PIRE_HIP_AFFIX_LONGEST 1u         /* LongestPrefix / LongestSuffix; without it the Shortest forms */
#define PIRE_HIP_AFFIX_THROUGH_BEGIN 2u   /* the reference's throughBeginMark */
#define PIRE_HIP_AFFIX_THROUGH_END 4u     /* the reference's throughEndMark */

/*
 * pire_hip_prefix on `head`, pire_hip_suffix on `tail` and pire_hip_affix_select, on one stream.  head and tail may each be
 * NULL (that scan is skipped and the pass gets no such array), not both; they may be the same table.  head_opts / tail_opts:
 * PIRE_HIP_AFFIX_* bits, the scans' longest, through_begin and through_end.  flags: PIRE_HIP_RUN_ON_DEVICE as above;
 * PIRE_HIP_RUN_GENERIC is handed to the prefix scan.  out_head_len[n], out_tail_len[n] (nullable): what the scans wrote;
 * what the caller has no array for lives in stream-ordered scratch of the library's own.  part, out_hits, out_spans, hit_cap,
 * out_hit_count: as pire_hip_affix_select.  With host pointers the text is staged once, and both scans and the pass run on
 * the staged copy before anything comes back.  Each scan keeps its first-use self-test and its kernel choice;
 * pire_hip_last_kernel() names the scan that ran last.  It refuses what the three calls it stands for refuse (a part that
 * needs the table that is NULL; unknown bits in head_opts or tail_opts).
 */
int pire_hip_affix_run_select(pire_hip_table* head, uint32_t head_opts, pire_hip_table* tail, uint32_t tail_opts,
                              const void* text, const uint64_t* offsets, uint64_t n, uint32_t part, uint32_t flags,
                              int64_t* out_head_len, int64_t* out_tail_len,
                              uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);

/*
 * Raw bytes in, the matched head or tail of every line that matched -- or the line without them -- out: `grep -o '^re'`,
 * `sed 's/^re//'` on the lines that match, a trim of both ends in one call.  The split into scratch, the scans on the lines,
 * the pass -- its spans counted in raw: line i of the split buffer lies i bytes further into raw --, the gather from raw
 * through them.  head .. tail_opts, part: as pire_hip_affix_run_select.  Everything else as pire_hip_capture_lines_gather:
 * out_line_count, delim, the one synchronisation of `stream`, the refusal of 2^32 lines (PIRE_HIP_EUNSUPPORTED); out_hits
 * (nullable): the numbers of the lines that matched; out_spans (nullable): byte ranges of raw; tail_byte (the gather's
 * `tail`), out_text, text_cap, out_offsets (hit_cap + 1 entries), out_bytes: as pire_hip_gather_spans.  All four gather outputs null (text_cap == 0):
 * spans only, the gather is skipped.  Host pointers with size == 0: zeros (out_offsets[0] = 0 where it is not null), no
 * device is touched.
 */
int pire_hip_affix_lines_gather(pire_hip_table* head, uint32_t head_opts, pire_hip_table* tail, uint32_t tail_opts,
                                const void* raw, uint64_t size, uint32_t delim, uint32_t part, uint32_t flags, uint32_t tail_byte,
                                uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_spans,
                                uint64_t hit_cap, uint64_t* out_hit_count,
                                void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes,
                                void* stream);

/* ---- where the match lies: leftmost-longest spans, on the device ------------------------------------------------------ */

#define PIRE_HIP_SEARCH_SHORTEST 1u        /* S: the forward leg is ShortestPrefix; without it LongestPrefix */
#define PIRE_HIP_SEARCH_THROUGH_BEGIN 2u   /* B: the reference's throughBeginMark */
#define PIRE_HIP_SEARCH_THROUGH_END 4u     /* E: the reference's throughEndMark */

/*
 * Where the leftmost-longest match of a regexp `re` lies inside every string of a batch: two searches of the reference's
 * run.h, composed in ONE launch.  The caller holds two Pire::Scanners that are not Surround()ed, as tables:
 *   fwd (F)  compiled from `re`
 *   rev (R)  compiled from Fsm::Reverse() of `re` followed by `.*`
 * For string i = text[offsets[i], offsets[i+1]) of length len_i (offsets[i+1] < offsets[i]: a string of length 0, as in
 * pire_hip_affix_select), with the bits of opts B = THROUGH_BEGIN, E = THROUGH_END, S = SHORTEST:
 *   t_i   = LongestSuffix(R, string i, throughEndMark = E, throughBeginMark = B)     length, or -1          run.h:313-341
 *   b_i   = len_i - t_i                                                              the leftmost start
 *   h_i   = S ? ShortestPrefix(F, string i from b_i, throughBeginMark = B && b_i == 0, throughEndMark = E)
 *             : LongestPrefix (F, string i from b_i, ...the same...)                 length, or -1          run.h:277-311
 *   found(i) = t_i >= 0 && h_i >= 0
 *   begin[i] = found ? b_i : -1        end[i] = found ? b_i + h_i : -1              positions inside the string
 * An empty match is a match: begin == end.  The semantics are POSIX's leftmost-longest, not the leftmost-first of
 * backtracking engines: `abc|abcabc|b+` on `abcabc` gives [0, 6).  t_i >= 0 with h_i < 0 can only happen when the two tables
 * do not belong together; the string is then not found, and nothing else is promised for such a pair.  rev and fwd may be
 * the same table.
 * out_begin[n], out_end[n] (required): written for all n strings.  n < 2^32.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> text, offsets and the outputs are device pointers and the call only enqueues on `stream`:
 *        one kernel, one string per lane, 1 024-thread blocks that hold both tables' dense rows in LDS.  Otherwise host
 *        pointers: the batch is staged once and the call synchronises.
 * PIRE_HIP_EINVAL before any device is touched: null rev or fwd; unknown bits in opts; n > 0 with null text or offsets; null
 * out_begin or out_end; n >= 2^32.  PIRE_HIP_EUNSUPPORTED before anything is launched where the two tables' dense rows do
 * not fit the LDS of a block (two tables of 255 dense rows take 137 312 bytes; not on a device with 160 KiB).
 * pire_hip_last_kernel() is not changed by the search.  No first-use self-test.
 */
int pire_hip_search(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts,
                    const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                    int64_t* out_begin, int64_t* out_end, void* stream);

/*
 * pire_hip_search and, behind it on the same stream, pire_hip_capture_select without the BeginMark shift and without
 * need_final: begin[i] and end[i] are exactly that pass's input -- found <=> both >= 0, spans clamped into the string.
 * out_begin[n], out_end[n] (nullable): what the search wrote; what the caller has no array for lives in stream-ordered
 * scratch of the library's own.  out_hits, out_spans, hit_cap, out_hit_count: as pire_hip_capture_select.  With host
 * pointers the batch is staged once, and the search and the pass run on the staged copy before anything comes back.  It
 * refuses what pire_hip_search refuses (the null result arrays excepted) and what pire_hip_capture_select refuses of its
 * outputs.
 */
int pire_hip_search_run_select(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts,
                    const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                    int64_t* out_begin, int64_t* out_end,
                    uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);

/*
 * Raw bytes in, the first (leftmost-longest) match of every line that has one out -- with tail_byte = delim, `grep -o` for
 * the first match of each line.  The split into scratch, the search on the lines, the pass -- its spans counted in raw: line
 * i of the split buffer lies i bytes further into raw --, the gather from raw through them.  rev, fwd, opts: as
 * pire_hip_search.  Everything else as pire_hip_capture_lines_gather: out_line_count, delim, the one synchronisation of
 * `stream`, the refusal of 2^32 lines (PIRE_HIP_EUNSUPPORTED); out_hits (nullable): the numbers of the lines with a match;
 * out_spans (nullable): byte ranges of raw; tail_byte (the gather's `tail`), out_text, text_cap, out_offsets (hit_cap + 1
 * entries), out_bytes: as pire_hip_gather_spans.  All four gather outputs null (text_cap == 0): spans only, the gather is
 * skipped.  flags: PIRE_HIP_RUN_ON_DEVICE; the marks are opts', other bits are ignored.  Host pointers with size == 0: zeros (out_offsets[0] = 0 where it is not
 * null), no device is touched.
 */
int pire_hip_search_lines_gather(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts,
                    const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint32_t tail_byte,
                    uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_spans, uint64_t hit_cap, uint64_t* out_hit_count,
                    void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* stream);

/*
 * EVERY leftmost-longest match of every string, not the first alone: the two searches of pire_hip_search, iterated.  rev (R),
 * fwd (F) and opts (S, B, E) are exactly as for pire_hip_search.  For string s of length len:
 *   p = 0, k = 0
 *   while p < len:
 *       t = LongestSuffix(R, s[p, len), throughEndMark = E, throughBeginMark = B && p == 0)      run.h:313-341
 *       if t <= 0: stop                      (t == 0: only the empty match at len is left)
 *       b = len - t
 *       h = S ? ShortestPrefix(F, s[b, len), throughBeginMark = B && b == 0, throughEndMark = E)
 *             : LongestPrefix (F, ...the same...)                                                 run.h:277-311
 *       if h < 0: stop                       (two tables that do not belong together)
 *       if h > 0: match k of the string = [b, b + h);  k += 1
 *       p = b + max(h, 1)
 * The matches of a string do not overlap and they ascend.  An empty match is never reported (`grep -o` drops it too); the
 * walk steps one byte past it.  `^` matches at byte 0 only: B is handed to a leg only at byte 0.  The first reported match
 * is pire_hip_search's wherever that one is not empty.
 * The device does not run one backward search per match: R's state after the bytes len-1 .. j does not depend on p, so
 *   LongestSuffix(R, s[p, len)) = len - min{ j >= p : mark(j) }
 *   mark(j) = Final(state after byte j) || (j == 0 && B && Final(Step(that state, BeginMark)))
 * with no marks below the position where the walk reached a Dead state: one backward pass writes the marks, one bit per byte
 * of text in stream-ordered scratch of 2 * (text_bytes / 16 + n + 2) bytes.  The forward leg walks until F is Dead
 * (LongestPrefix's rule): a pattern such as `a.*b|a` on a line of `a`s without a `b` costs len steps per match, len^2 for
 * the line.  That is the definition's cost, not the kernel's.
 * text_bytes: the size of the buffer behind `text`; the caller promises that every offset is <= text_bytes.  The kernels clamp
 * whatever is larger, so nothing outside the scratch or the text is touched.  Offsets must not decrease; where
 * offsets[i+1] < offsets[i], string i is empty (as in pire_hip_search).  Strings that OVERLAP in text (which takes such a
 * decrease) get unspecified matches -- their marks share words --, but nothing is accessed out of bounds.
 * out_rows[n + 1] (nullable): CSR row starts, the matches of string i are entries [rows[i], rows[i+1]) of the lists.  Never
 *        capped: rows[n] = the match count.
 * out_owners[match_cap] (nullable): the string of match k; ascending, with repeats.
 * out_spans[2 * match_cap] (nullable): match k as a byte range of text, (offsets[i] + b, offsets[i] + b + h): the convention of
 *        pire_hip_capture_select, the input form of pire_hip_gather_spans.
 * out_match_count (required): the number of matches, also where it exceeds match_cap; then the first match_cap entries of
 *        the lists are written and nothing beyond them.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> everything is a device pointer, the call only enqueues on `stream` (four launches) and
 *        does not wait.  Otherwise host pointers: the batch is staged once and the call synchronises.
 * PIRE_HIP_EINVAL before any device is touched: null rev or fwd; unknown bits in opts; n > 0 with null text or offsets;
 * n >= 2^32; null out_match_count; match_cap > 0 with null out_owners and null out_spans; host pointers: offsets that
 * decrease, or an offset beyond text_bytes.  PIRE_HIP_EUNSUPPORTED as pire_hip_search (the dense rows and the LDS).
 * n == 0: the count is 0 (and rows[0]); device pointers: zeroed on the stream; host pointers: no device is touched.
 * pire_hip_last_kernel() is not changed.  No first-use self-test.
 */
int pire_hip_search_all(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts,
                    const void* text, uint64_t text_bytes, const uint64_t* offsets, uint64_t n, uint32_t flags,
                    uint64_t* out_rows, uint64_t* out_owners, uint64_t* out_spans, uint64_t match_cap,
                    uint64_t* out_match_count, void* stream);

/*
 * Raw bytes in, every match of every line out -- with tail_byte = delim, `grep -o`'s output byte for byte.  As
 * pire_hip_search_lines_gather, with the list form of the search: a line can have many matches, so the lists are match_cap
 * long (not min(match_cap, lines)).  out_owners (nullable): the line number of match k; out_spans (nullable): byte ranges of
 * raw (line i of the split buffer lies i bytes further into raw); out_match_count: the matches, also beyond match_cap.  The
 * gather runs straight from raw through the spans, tail_byte behind each match; all four gather outputs null: spans only.
 * The matches do not overlap, so size + match_cap bytes of out_text always suffice.  One synchronisation of `stream`; 2^32
 * lines are refused (PIRE_HIP_EUNSUPPORTED).  Host pointers with size == 0: zeros, no device is touched.
 */
int pire_hip_search_all_lines_gather(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts,
                    const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint32_t tail_byte,
                    uint64_t* out_line_count, uint64_t* out_owners, uint64_t* out_spans, uint64_t match_cap, uint64_t* out_match_count,
                    void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* stream);

/* ---- labelled matches and tokens, on the device ------------------------------------------------------------------ */

#define PIRE_HIP_LEX_SHORTEST 1u       /* = PIRE_HIP_SEARCH_SHORTEST */
#define PIRE_HIP_LEX_THROUGH_BEGIN 2u  /* = PIRE_HIP_SEARCH_THROUGH_BEGIN */
#define PIRE_HIP_LEX_THROUGH_END 4u    /* = PIRE_HIP_SEARCH_THROUGH_END */
#define PIRE_HIP_LEX_TOKENS 8u         /* maximal-munch tokens and the gaps between them, through fwd alone */

/*
 * Which regexp each match belongs to: Scanner::Glue followed by AcceptedRegexps, per MATCH instead of per string.
 * fwd (F): a glued Scanner of R regexps re_0 .. re_{R-1}, 1 <= R <= 64, not Surround()ed.  rev (R~): the Scanner of
 * `((re_0)|(re_1)|...)` followed by the lexer's `.*`, compiled from Fsm::Reverse() -- MatchFinder's construction over the
 * union.  opts: S, B, E with the values and the meaning of PIRE_HIP_SEARCH_*, and PIRE_HIP_LEX_TOKENS.
 *
 * SEARCH MODE (no TOKENS) is exactly pire_hip_search_all's loop over rev and fwd: spans, owners and rows are bit for bit what
 * that call writes for the same tables.  Every reported match k also gets mask[k]:
 *   q = F's state after the h bytes of the match, from Initialize() (+ Step(BeginMark) where the leg took the mark)
 *   mask = AcceptedRegexps(q) as bits                                  if Final(q)
 *   mask |= AcceptedRegexps(Step(q, EndMark)) as bits                  if E, the match ends at len and Final(Step(q, EndMark))
 * The mask of a reported match is never 0.
 *
 * TOKEN MODE (TOKENS) does not use rev, which may be null; no mark pass, no mark scratch.  For string s of length len:
 *   p = 0
 *   while p < len:
 *       h = S ? ShortestPrefix(F, s[p, len), throughBeginMark = B && p == 0, throughEndMark = E)
 *             : LongestPrefix (F, ...the same...)                                                 run.h:277-311
 *       if h > 0: an entry [p, p + h) with its mask as above;  p += h
 *       else:     byte p is a gap byte;  p += 1
 *   a maximal run of gap bytes is ONE entry with mask 0
 * The entries of a string tile [0, len) exactly, in ascending order; an empty string has none.  Without E, dropping the gaps
 * leaves search mode's list.  With E, search mode only sees matches that accept through the EndMark (as pire_hip_search);
 * token mode is how to get a per-token `$`.  The walk restarts at every gap byte: a pattern whose forward leg runs far before
 * it fails (`a.*b`) costs that run per gap byte -- the definition's cost.
 *
 * text, text_bytes, offsets, n, flags, out_rows, out_owners, out_spans, match_cap, out_match_count: as pire_hip_search_all
 * (entries instead of matches), clamping, decreasing offsets and n == 0 included.
 * out_masks[match_cap] (nullable): the mask of entry k.
 * out_label_counts[R + 1] (nullable): entry r = the number of entries whose LOWEST set bit is r (lex's first-rule-wins), entry
 *        R = the number of gaps.  Counted over all entries, also beyond match_cap; exact 64-bit integers, the same for the
 *        same input.
 * PIRE_HIP_EINVAL before any device is touched: unknown bits in opts; null fwd; null rev without TOKENS; match_cap > 0 with
 * null out_owners, out_spans and out_masks; a SimpleScanner table; and what pire_hip_search_all refuses of its batch.
 * PIRE_HIP_EUNSUPPORTED before any device is touched: a fwd of more than 64 regexps (it has no accept masks).
 * PIRE_HIP_EUNSUPPORTED: the dense rows do not fit the LDS (token mode: F's alone count).
 * pire_hip_last_kernel() is not changed.  No first-use self-test.  Four launches on `stream`.
 */
int pire_hip_lex(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts,
                    const void* text, uint64_t text_bytes, const uint64_t* offsets, uint64_t n, uint32_t flags,
                    uint64_t* out_rows, uint64_t* out_owners, uint64_t* out_spans, uint64_t* out_masks, uint64_t match_cap,
                    uint64_t* out_match_count, uint64_t* out_label_counts, void* stream);

/*
 * Raw bytes in, every labelled match (or token) of every line out: split, pire_hip_lex on the lines, then the gather from raw
 * through the spans with tail_byte behind each entry.  As pire_hip_search_all_lines_gather, plus out_masks[match_cap] and
 * out_label_counts[R + 1] (both nullable).  Spans are byte ranges of raw.  In token mode the gathered entries of a line are
 * the line itself, cut.  size + match_cap bytes of out_text always suffice.  One synchronisation of `stream`; 2^32 lines are
 * refused (PIRE_HIP_EUNSUPPORTED).  Host pointers with size == 0: zeros (the label counts too), no device is touched.
 */
int pire_hip_lex_lines_gather(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts,
                    const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint32_t tail_byte,
                    uint64_t* out_line_count, uint64_t* out_owners, uint64_t* out_spans, uint64_t* out_masks, uint64_t match_cap,
                    uint64_t* out_match_count, uint64_t* out_label_counts,
                    void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes, void* stream);

/* ---- the matches replaced, on the device ------------------------------------------------------------------------- */

#define PIRE_HIP_SPLICE_KEEP 1u        /* the match itself stays, between head and tail */
#define PIRE_HIP_SPLICE_FIRST 2u       /* the lines form: the first match of every line (pire_hip_search), not every match */
#define PIRE_HIP_SPLICE_PIECE_MAX 256u /* head and tail: at most this many bytes each */

/*
 * The mirror image of pire_hip_gather_spans: the gather keeps the spans and drops the rest, this keeps the rest and puts a
 * piece where every span was -- `sed 's/re/repl/g'` (head = repl), deletion (no head, no tail), redaction, and with KEEP
 * `grep --color` or `sed 's/re/<b>&<\/b>/g'`.  It takes no table and no scan: it reads what pire_hip_search_all,
 * pire_hip_search_run_select, pire_hip_capture_select, pire_hip_affix_select or the slow capture pass wrote.
 *   k = min(span_count ? *span_count : span_cap, span_cap)
 *   [b_j, e_j) = [spans[2j], spans[2j+1])                      span j of raw, 0 <= j < k
 *   b_j <= e_j <= size,  e_{j-1} <= b_j                        ascending and disjoint; b_j == e_j: an insertion point
 *   piece_j = head ++ (KEEP ? raw[b_j, e_j) : "") ++ tail      P_j = |piece_j|
 *   out = raw[0, b_0) ++ piece_0 ++ raw[e_0, b_1) ++ piece_1 ++ ... ++ piece_{k-1} ++ raw[e_{k-1}, size)
 *   D(j) = sum over i < j of (P_i - (e_i - b_i))               64-bit, wrap-around
 *   *out_bytes = size + D(k)
 *   out_pos[j] = b_j + D(j)                                    where piece j begins in out
 *   out_offsets[i] = offsets[i] + D(first j with b_j >= offsets[i])        (that j is k where there is none)
 * Several empty spans at one position insert in list order.  k == 0: out is a copy of raw; size == 0: the pieces alone.
 * out_bytes (required): the whole need, also beyond text_cap; only the bytes of out_text at positions < text_cap are written.
 * out_pos[span_cap] (nullable): entries [0, k) are written and nothing behind them.  Where it is null the pass keeps them in
 *        stream-ordered scratch of 8 * span_cap bytes; where it is not, the pass allocates nothing.
 * offsets[n + 1], out_offsets[n + 1] (nullable together): string boundaries in raw, not decreasing, <= size, and where they
 *        lie in out.  A span belongs to the string it begins in, an empty span on a boundary to the string that BEGINS there
 *        -- so an empty match at the very end of string i-1 moves to string i (the one odd case; it does not arise in the
 *        lines forms, where a delimiter lies between two lines).  The caller promises that no span straddles a boundary.
 * head, tail: HOST memory in every mode, head_len and tail_len <= PIRE_HIP_SPLICE_PIECE_MAX, read before the call returns.
 *        They travel as kernel arguments: the device form allocates nothing for them and stays legal inside a stream capture.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> every other pointer is a device pointer, the call only enqueues on `stream` (four
 *        launches) and does not wait.  Otherwise host pointers: staged once, and the call synchronises.  Not in place.
 * PIRE_HIP_EINVAL before any device is touched: null out_bytes; head_len or tail_len > 256; a length > 0 with a null pointer;
 * unknown bits in mode (FIRST is the lines form's); span_cap > 0 with null spans; text_cap > 0 with null out_text; exactly one
 * of offsets / out_offsets null; size > 0 with null raw; span_cap >= 2^32 or n >= 2^32; out_text[0, text_cap) overlapping
 * raw[0, size); host pointers: a list that is not ascending and disjoint or leaves [0, size], offsets that decrease or
 * exceed size.
 * Device pointers and a list that breaks the promise: the output bytes and *out_bytes are unspecified, but nothing is read
 * outside raw[0, size) or the lists and nothing is written outside out_text[0, text_cap), out_pos[0, k), out_offsets[0, n]
 * and out_bytes: every source position is clamped (the rule pire_hip_search_all has for strings that overlap).
 * pire_hip_last_kernel() is not changed.  No first-use self-test.
 */
int pire_hip_splice(const void* raw, uint64_t size,
                    const uint64_t* spans, const uint64_t* span_count, uint64_t span_cap,
                    const void* head, uint32_t head_len, const void* tail, uint32_t tail_len, uint32_t mode,
                    const uint64_t* offsets, uint64_t n, uint32_t flags,
                    void* out_text, uint64_t text_cap, uint64_t* out_pos, uint64_t* out_offsets,
                    uint64_t* out_bytes, void* stream);

/*
 * Raw bytes in, rewritten bytes out -- `sed 's/re/repl/g'` on a resident buffer: the split, the search on the lines, the
 * splice straight over raw.  The delimiters are kept text, so out_text is the buffer as sed would print it and can be split
 * again.  rev, fwd, opts as pire_hip_search; head, tail, mode as pire_hip_splice.
 * Without PIRE_HIP_SPLICE_FIRST: the list form of the search (pire_hip_search_all), lists match_cap long.  An empty match is
 *        never replaced -- the list form never reports one --, so `sed 's|x*|-|g'`, which also inserts at every empty
 *        match, differs here: only the runs of x are replaced.
 * With FIRST: pire_hip_search's first match of every line; an empty first match is an insertion, as in sed (`s/^/> /`).  The
 *        lists are min(match_cap, lines) long.
 * out_line_count, out_match_count (required): the lines, and the matches found -- also beyond match_cap; then only the first
 *        match_cap matches are replaced and the rest of the text is copied as it is: the caller sees the need and retries.
 * out_spans[2 * match_cap], out_pos[match_cap] (nullable): the replaced ranges of raw and where their pieces begin in
 *        out_text; where null the library keeps them in scratch.
 * out_bytes (required), out_text[text_cap]: as pire_hip_splice.  size + match_cap * (head_len + tail_len) bytes always suffice.
 * It refuses what pire_hip_search_all_lines_gather refuses of its inputs and what pire_hip_splice refuses of its outputs.  One
 * synchronisation of `stream`; 2^32 lines are refused (PIRE_HIP_EUNSUPPORTED).  Host pointers with size == 0: zeros, no
 * device is touched.
 */
int pire_hip_search_lines_splice(pire_hip_table* rev, pire_hip_table* fwd, uint32_t opts,
                    const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                    const void* head, uint32_t head_len, const void* tail, uint32_t tail_len, uint32_t mode,
                    uint64_t* out_line_count, uint64_t* out_spans, uint64_t* out_pos, uint64_t match_cap,
                    uint64_t* out_match_count, void* out_text, uint64_t text_cap, uint64_t* out_bytes, void* stream);

/* ---- the strings that count, on the device ---------------------------------------------------------------------- */

/*
 * From result rows to the strings whose counters reach their thresholds -- a compacted, ascending list of their indices and
 * rows -- and the occurrences of every regexp over the batch.  It takes no table and no text: it reads what
 * pire_hip_counting_run or pire_hip_run_half_final wrote (results[n][regexps]), behind any of the counting kernels.  With
 * R = regexps and c(i, r) = results[i * R + r]:
 *   m(r)        = min_count ? min_count[r] : 1                  min_count (nullable): R entries
 *   wanted(r)   = m(r) > 0
 *   pass(i, r)  = c(i, r) >= m(r)
 *   selected(i) = some wanted r passes                          (default, ANY)
 *   selected(i) = some r is wanted and every wanted r passes    (mode & PIRE_HIP_COUNT_ALL)
 * With no wanted r nothing is selected.
 * out_totals[R] (nullable): the sum of c(i, r) over ALL n strings, selected or not, exact in 64 bits; written, not
 * accumulated; n == 0 writes R zeros.  out_hits[hit_cap] (nullable): the indices of the selected strings, ascending.
 * out_hit_results[hit_cap][R] (nullable, and it does not need out_hits): the result row of hit k.  *out_hit_count
 * (required): the number of selected strings, also when it exceeds hit_cap; only the first min(count, hit_cap) entries of
 * the two lists are written, nothing behind them.  R == 0: PIRE_HIP_OK, a count of 0 and nothing else written.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> every pointer (min_count included) is a device pointer and the call only enqueues on
 *        `stream`: classify per tile of 1 024 strings, the one-block scan of pire_hip_select, scatter and -- for out_totals --
 *        one uint64 sum per tile and regexp and their reduction; no atomics, no block waits for another: the same input gives
 *        the same bits.  Scratch (n / 8 + n / 256 bytes, + R * ceil(n / 1024) * 8 for the totals) comes from the
 *        stream-ordered allocator: the rule and the capture-mode caveat stated at pire_hip_select.  `results` needs 4-byte
 *        alignment only.  Otherwise host pointers: staged, synchronises, the lists come back only as far as they were written.
 * PIRE_HIP_EINVAL before any device is touched: null out_hit_count; n > 0 and R > 0 with null results; unknown bits in
 * mode; hit_cap > 0 with null out_hits and null out_hit_results.  PIRE_HIP_EUNSUPPORTED: n >= 2^32, R > 1024.
 * pire_hip_last_kernel() is not changed by the pass.  No first-use self-test (as pire_hip_select).
 */
#define PIRE_HIP_COUNT_ALL 0x1u      /* in `mode` */
int pire_hip_count_select(const uint32_t* results, uint64_t n, uint32_t regexps, const uint32_t* min_count, uint32_t mode,
                          uint32_t flags, uint64_t* out_totals, uint64_t* out_hits, uint32_t* out_hit_results,
                          uint64_t hit_cap, uint64_t* out_hit_count, void* stream);

/*
 * pire_hip_counting_run / pire_hip_run_half_final followed by pire_hip_count_select on the same stream, behind whichever
 * kernel the scan takes.  t .. out_results: as the run call; R is the table's.  out_results is nullable here: the rows then
 * live in stream-ordered scratch of the library's own.  With host pointers the text is staged once, and scan and pass run
 * on the staged copy before anything comes back.  Hit indices are relative to the whole batch.  They refuse what the run
 * call refuses (the null out_results excepted) and what pire_hip_count_select refuses.  pire_hip_last_kernel() names the
 * scan's kernel.
 */
int pire_hip_counting_run_select(pire_hip_counting_table* t, int kind, const void* text, const uint64_t* offsets, uint64_t n,
                                 uint32_t flags, uint32_t* out_state_idx, uint32_t* out_results,
                                 const uint32_t* min_count, uint32_t mode, uint64_t* out_totals, uint64_t* out_hits,
                                 uint32_t* out_hit_results, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);
int pire_hip_run_half_final_select(pire_hip_table* t, const void* text, const uint64_t* offsets, uint64_t n, uint32_t flags,
                                   uint32_t* out_state_idx, uint8_t* out_final, uint32_t* out_results,
                                   const uint32_t* min_count, uint32_t mode, uint64_t* out_totals, uint64_t* out_hits,
                                   uint32_t* out_hit_results, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);

/*
 * Raw bytes in, the lines that count out: the split into scratch, the counting scan on the lines with the rows in scratch,
 * the pass.  out_line_count (required), delim, the one synchronisation of `stream` (the split's; the call adds none) and
 * the refusal of 2^32 lines: as pire_hip_run_lines_select.  min_count, mode, out_totals, out_hits (the numbers of the
 * lines), out_hit_results, hit_cap, out_hit_count: as pire_hip_count_select.  out_hit_spans[hit_cap][2] (nullable, needs
 * out_hits): the whole line of hit k as a byte range of raw, delimiter not included -- the input of pire_hip_gather_spans,
 * which chains on it with device pointers (the gather stays the caller's).  Host pointers with size == 0: zeros, no device
 * is touched.  They also refuse delim > 255, null out_line_count and size > 0 with null raw.
 */
int pire_hip_counting_lines_select(pire_hip_counting_table* t, int kind, const void* raw, uint64_t size, uint32_t delim,
                                   uint32_t flags, const uint32_t* min_count, uint32_t mode, uint64_t* out_line_count,
                                   uint64_t* out_totals, uint64_t* out_hits, uint64_t* out_hit_spans,
                                   uint32_t* out_hit_results, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);
int pire_hip_half_final_lines_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                     const uint32_t* min_count, uint32_t mode, uint64_t* out_line_count,
                                     uint64_t* out_totals, uint64_t* out_hits, uint64_t* out_hit_spans,
                                     uint32_t* out_hit_results, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);

/* ---- the lines around a match, on the device (grep -A / -B / -C) -------------------------------------------------- */

/*
 * From a hit list to the hits and their neighbours: the ascending list of the lines that lie within `after` lines behind or
 * `before` lines in front of a hit, and two bits a line.  It takes no table and no text: it reads line numbers, whoever wrote
 * them -- every hit pass of the library writes such a list.  With k = min(hit_count ? *hit_count : hit_cap, hit_cap) (as
 * pire_hip_gather) and hits[0, k) strictly ascending, every entry < n:
 *   selected(i) <=> 0 <= i < n and there is j < k with hits[j] - before <= i <= hits[j] + after
 * over the integers: nothing wraps, every value of before and after is legal, 2^64 - 1 included; before = after = 0 gives the
 * hit list back.  out_lines[line_cap] (nullable): the selected i, ascending.  out_line_flags[line_cap] (nullable, needs
 * out_lines): for out_lines[r],
 *   PIRE_HIP_CONTEXT_HIT    the line is itself in the hit list (grep -n prints ':' behind its number, else '-')
 *   PIRE_HIP_CONTEXT_GROUP  i == 0 or line i - 1 is not selected: the first line of a run (where grep prints "--" in front,
 *                           the first run excepted)
 * *out_line_count (required): the number of selected lines, also when it exceeds line_cap; only the first
 * min(count, line_cap) entries of the two lists are written, nothing behind them.  *out_group_count (nullable): the number of
 * selected lines that carry PIRE_HIP_CONTEXT_GROUP.  n == 0 or k == 0: both counts are 0, nothing else is written.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> every pointer (hit_count included) is a device pointer and the call only enqueues on
 *        `stream`: classify per tile of 1 024 LINES -- a hit with after = 10^6 costs what any other costs --, the one-block
 *        scan of pire_hip_select (a second launch of it for out_group_count), scatter; no atomics, no block waits for
 *        another: the same input gives the same bits.  Scratch (3 * n / 8 + n / 128 bytes) comes from the stream-ordered
 *        allocator: the rule and the capture-mode caveat stated at pire_hip_select.  `hits` and out_line_flags may have any
 *        alignment.  A list that is not ascending, or that names lines >= n, gives an unspecified selection; even then the
 *        call reads nothing outside hits[0, k) and writes nothing outside what is stated above.  Otherwise host pointers:
 *        staged, synchronises, the lists come back only as far as they were written; a list that is not strictly ascending or
 *        that names a line >= n is PIRE_HIP_EINVAL, and nothing is written.
 * PIRE_HIP_EINVAL before any device is touched: null out_line_count; hit_cap > 0 with null hits; line_cap > 0 with null
 * out_lines; out_line_flags without out_lines; n >= 2^32; hit_cap >= 2^32.
 * pire_hip_last_kernel() is not changed by the pass.  No first-use self-test: it takes no table (as pire_hip_split).
 *
 * The chain that serves every lines form with device pointers and no read-back: pire_hip_split with out_text == NULL (the
 * offsets of the lines in raw), any hit list over those lines, pire_hip_context, pire_hip_gather over raw and the split's
 * offsets with idx = out_lines, idx_count = out_line_count and PIRE_HIP_GATHER_NO_TAIL (an offset range of the split with
 * out_text == NULL includes the line's delimiter).
 */
#define PIRE_HIP_CONTEXT_HIT   1u   /* out_line_flags: the line is itself in the hit list */
#define PIRE_HIP_CONTEXT_GROUP 2u   /* out_line_flags: line 0, or line i - 1 is not selected: the first line of a run */
int pire_hip_context(const uint64_t* hits, const uint64_t* hit_count, uint64_t hit_cap, uint64_t n,
                     uint64_t before, uint64_t after, uint32_t flags,
                     uint64_t* out_lines, uint8_t* out_line_flags, uint64_t line_cap,
                     uint64_t* out_line_count, uint64_t* out_group_count, void* stream);

/*
 * Raw bytes in, the lines that match and their neighbours out: `grep -A after -B before`.  The split into scratch, the scan
 * on the lines with its hit list in stream-ordered scratch (8 bytes a line at most), pire_hip_context on that list; the
 * context list takes the place the hit list has in pire_hip_run_lines_select / _gather and pire_hip_slow_lines_select /
 * _gather, whose t, raw, size, delim, flags, want / mode, out_line_count, one synchronisation of `stream` and refusal of 2^32
 * lines these forms keep (mode PIRE_HIP_FINAL_SELECT_ZERO: `grep -v -C`).  out_lines[line_cap], out_line_flags[line_cap],
 * *out_group_count: as pire_hip_context.  out_line_spans[line_cap][2] (nullable, needs out_lines): the whole line of
 * out_lines[r] as a byte range of raw, delimiter not included.  *out_sel_count (required): the number of selected lines,
 * pire_hip_context's out_line_count.  *out_hit_count (nullable): the number of lines that matched (`grep -c`).
 * The gather forms: out_lines is nullable (the list then lives in scratch of the library's own); tail, out_text, text_cap,
 * out_offsets (line_cap + 1 entries), out_bytes: as pire_hip_gather_spans.  With tail = delim out_text holds what
 * `grep -A after -B before --no-group-separator` prints; the "--" lines are the caller's to insert, PIRE_HIP_CONTEXT_GROUP
 * says where.  They refuse what the form they extend refuses, what pire_hip_context refuses and, of their outputs, what
 * pire_hip_gather_spans refuses.  Host pointers with size == 0: zeros (out_offsets[0] = 0 where it is not null), no device
 * is touched.
 */
int pire_hip_run_lines_context_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                      const uint64_t* want, uint64_t before, uint64_t after, uint64_t* out_line_count,
                                      uint64_t* out_lines, uint8_t* out_line_flags, uint64_t* out_line_spans, uint64_t line_cap,
                                      uint64_t* out_sel_count, uint64_t* out_group_count, uint64_t* out_hit_count, void* stream);
int pire_hip_run_lines_context_gather(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                      const uint64_t* want, uint64_t before, uint64_t after, uint64_t* out_line_count,
                                      uint64_t* out_lines, uint8_t* out_line_flags, uint64_t* out_line_spans, uint64_t line_cap,
                                      uint64_t* out_sel_count, uint64_t* out_group_count, uint64_t* out_hit_count,
                                      uint32_t tail, void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes,
                                      void* stream);
int pire_hip_slow_lines_context_select(pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                       uint32_t mode, uint64_t before, uint64_t after, uint64_t* out_line_count,
                                       uint64_t* out_lines, uint8_t* out_line_flags, uint64_t* out_line_spans, uint64_t line_cap,
                                       uint64_t* out_sel_count, uint64_t* out_group_count, uint64_t* out_hit_count, void* stream);
int pire_hip_slow_lines_context_gather(pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                       uint32_t mode, uint64_t before, uint64_t after, uint64_t* out_line_count,
                                       uint64_t* out_lines, uint8_t* out_line_flags, uint64_t* out_line_spans, uint64_t line_cap,
                                       uint64_t* out_sel_count, uint64_t* out_group_count, uint64_t* out_hit_count,
                                       uint32_t tail, void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes,
                                       void* stream);

/* ---- hits by file, on the device (grep -c / -l / -L / -H -n over many files in one buffer) ------------------------------ */

/*
 * From a hit list and the files' line boundaries to the hits of every file.  It takes no table and no text: it reads line
 * numbers, whoever wrote them -- every hit pass of the library writes such a list.  With
 * k = min(hit_count ? *hit_count : hit_cap, hit_cap) (as pire_hip_context and pire_hip_gather), hits[0, k) strictly ascending
 * and every entry < n, and bounds[files + 1] non-decreasing with bounds[0] == 0 and bounds[files] == n: file f is the lines
 * [bounds[f], bounds[f + 1]); repeated bounds are empty files, legal anywhere and in any number.
 *   out_file_first[files + 1] (nullable): out_file_first[f] = the number of j < k with hits[j] < bounds[f].  The hits of file f
 *       are hits[first[f], first[f + 1]), their number is `grep -c`.
 *   out_hit_file[hit_cap], out_hit_line[hit_cap] (each nullable): for j < k the one f with bounds[f] <= hits[j] < bounds[f + 1],
 *       and hits[j] - bounds[f]: the line number inside the file, 0-based (`grep -n` prints it plus one).  Nothing is written at
 *       j >= k.
 *   out_files[file_cap] (nullable when file_cap == 0): the ascending list of the f with a hit (`grep -l`); with file_mode
 *       PIRE_HIP_FILES_WITHOUT the list of the f with none, empty files included (`grep -L`).
 *   *out_file_count (required): the length of that list, also when it exceeds file_cap; only the first min(count, file_cap)
 *       entries are written, nothing behind them.
 * files == 0 (n must be 0 then): the count is 0, out_file_first[0] = 0 where it is not null.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> every pointer (hit_count included) is a device pointer and the call only enqueues on
 *        `stream`: a lower bound in the list per file boundary (work is divided by files), classify per tile of 1 024 FILES, the
 *        one-block scan of pire_hip_select, scatter, and -- only where out_hit_file or out_hit_line is asked for -- locate per
 *        tile of 1 024 HITS: two wave-wide searches bound the slice of bounds a tile needs, so a tile inside one file costs
 *        those two and no more; no atomics, no block waits for another: the same input gives the same bits.  Scratch
 *        (files / 8 + files / 256 bytes, and 8 * (files + 1) where out_file_first is null) comes from the stream-ordered
 *        allocator: the rule and the capture-mode caveat stated at pire_hip_select.  `hits` may have any alignment, the other
 *        arrays are 8-byte aligned.  A list or bounds that break the preconditions give unspecified answers and nothing worse:
 *        the call reads nothing outside hits[0, k) and bounds[0, files] and writes nothing outside what is stated above.
 *        Otherwise host pointers: staged, synchronises, the file list comes back only as far as it was written; hits that are
 *        not strictly ascending or name a line >= n, bounds that decrease, bounds[0] != 0 and bounds[files] != n are
 *        PIRE_HIP_EINVAL, and nothing is written.
 * PIRE_HIP_EINVAL before any device is touched: null out_file_count; hit_cap > 0 with null hits; files > 0 with null bounds;
 * file_cap > 0 with null out_files; file_mode > 1; files == 0 with n > 0; n, hit_cap or files >= 2^32.
 * pire_hip_last_kernel() is not changed by the pass.  No first-use self-test: it takes no table (as pire_hip_context).
 *
 * The chain that gives the text of one file's hits -- or of all files' -- with device pointers and no read-back: a lines form
 * below (or any hit list with its spans), then pire_hip_gather_spans(raw, size, out_hit_spans + 2 * first[f], NULL,
 * first[f + 1] - first[f], ...) for file f, where the caller knows first[] -- or, for every file at once,
 * pire_hip_gather_spans(raw, size, out_hit_spans, out_hit_count, hit_cap, ...), whose out_offsets[first[f]] ..
 * out_offsets[first[f + 1]] are then file f's bytes of out_text.
 */
#define PIRE_HIP_FILES_WITHOUT 1u   /* file_mode: list the files with NO hit (grep -L) instead of those with one (grep -l) */
int pire_hip_files(const uint64_t* hits, const uint64_t* hit_count, uint64_t hit_cap, uint64_t n,
                   const uint64_t* bounds, uint64_t files, uint32_t file_mode, uint32_t flags,
                   uint64_t* out_file_first, uint64_t* out_hit_file, uint64_t* out_hit_line,
                   uint64_t* out_files, uint64_t file_cap, uint64_t* out_file_count, void* stream);

/*
 * The bytes of many files laid end to end in, the matching lines by file out: one call for `grep -c / -l / -L / -H -n
 * file...`.  file_bytes[files + 1], non-decreasing with file_bytes[0] == 0 and file_bytes[files] == size: file f is
 * raw[file_bytes[f], file_bytes[f + 1]).  The split, the scan, the hit list, the one synchronisation of `stream`, the refusals
 * and the refusal of 2^32 lines are those of pire_hip_run_lines_select / pire_hip_slow_lines_select (`want` chooses regexps;
 * mode PIRE_HIP_FINAL_SELECT_ZERO: `grep -v -c`, `grep -v -l`), as are out_line_count, out_hits, out_hit_spans, hit_cap and
 * out_hit_count.  On top of them:
 *   out_file_lines[files + 1] (nullable): out_file_lines[f] = the number of lines whose first byte lies in front of
 *       file_bytes[f] -- a line belongs to the file that holds its first byte.  These are the `bounds` of pire_hip_files.
 *   *out_straddles (required): the number of f in [1, files) with 0 < file_bytes[f] < size and
 *       raw[file_bytes[f] - 1] != delim: boundaries inside a line, because the file in front of them does not end in the
 *       delimiter.  0 for well-formed input; otherwise the answers are still those of the rule above, and the caller knows.
 *   out_hit_file[hit_cap], out_hit_line[hit_cap], out_file_first[files + 1], out_files[file_cap], *out_file_count: as
 *       pire_hip_files on the whole hit list (hit_cap cuts what is written, not what is counted) and out_file_lines.
 * They refuse what the form they extend refuses and, of the files, what pire_hip_files refuses (files == 0 with size > 0);
 * host-pointer calls refuse a bad file_bytes with PIRE_HIP_EINVAL before any device is touched.  Host pointers with
 * size == 0: zeros, out_file_first and out_file_lines all zero where not null, every file listed under
 * PIRE_HIP_FILES_WITHOUT; no device is touched.
 * There are no gather forms: out_hit_spans and out_file_first chain into pire_hip_gather_spans as stated at pire_hip_files.
 */
int pire_hip_run_lines_files_select(pire_hip_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                    const uint64_t* want, const uint64_t* file_bytes, uint64_t files, uint32_t file_mode,
                                    uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans, uint64_t* out_hit_file,
                                    uint64_t* out_hit_line, uint64_t hit_cap, uint64_t* out_hit_count, uint64_t* out_file_lines,
                                    uint64_t* out_file_first, uint64_t* out_files, uint64_t file_cap, uint64_t* out_file_count,
                                    uint64_t* out_straddles, void* stream);
int pire_hip_slow_lines_files_select(pire_hip_slow_table* t, const void* raw, uint64_t size, uint32_t delim, uint32_t flags,
                                     uint32_t mode, const uint64_t* file_bytes, uint64_t files, uint32_t file_mode,
                                     uint64_t* out_line_count, uint64_t* out_hits, uint64_t* out_hit_spans, uint64_t* out_hit_file,
                                     uint64_t* out_hit_line, uint64_t hit_cap, uint64_t* out_hit_count, uint64_t* out_file_lines,
                                     uint64_t* out_file_first, uint64_t* out_files, uint64_t file_cap, uint64_t* out_file_count,
                                     uint64_t* out_straddles, void* stream);

/* ---- boolean queries over hit lists, on the device (grep a | grep -v b, two columns, two kinds of scanner) -------------- */

/*
 * From up to six hit lists to the lines that a boolean function of "is in list j" selects.  It takes no table and no text: it
 * reads line numbers, whoever wrote them -- every hit pass of the library writes such a list, pire_hip_route one per regexp.
 * List j has k_j = min(list_counts && list_counts[j] ? *list_counts[j] : list_caps[j], list_caps[j]) entries (as
 * pire_hip_gather), lists[j][0, k_j) strictly ascending and every entry < n.  With
 *   m(i) = sum over j < k_lists of [i is in list j] << j,      for 0 <= i < n
 *   selected(i) <=> (truth >> m(i)) & 1
 * bits of truth at or above 2^k_lists are never looked at; bit 0 -- the lines in no list -- is legal: k_lists = 1 with
 * truth = 1 is the complement of a list (`grep -v` behind any pass), truth = 2 gives the list back, k_lists = 2 with
 * truth = 0x2 is "in list 0 and not in list 1", 0x8 the intersection, 0xE the union.
 *   out_hits[hit_cap] (nullable): the selected i, ascending.
 *   out_hit_members[hit_cap] (nullable, needs out_hits): m(out_hits[r]), one byte.
 *   *out_hit_count (required): the number of selected lines, also when it exceeds hit_cap; only the first
 *       min(count, hit_cap) entries of the two lists are written, nothing behind them.
 * n == 0: the count is 0, nothing else is written.  All lists empty: all n lines are selected if bit 0 of truth is set, none
 * otherwise.  The same list may be passed twice.
 * The arrays lists, list_counts (nullable as a whole: every k_j = list_caps[j]) and list_caps themselves, k_lists entries each,
 * are always HOST memory: they are read during the call and travel to the kernels by value.
 * flags: PIRE_HIP_RUN_ON_DEVICE -> their entries and all outputs are device pointers and the call only enqueues on `stream`
 *        -- the rows of pire_hip_route pass as they are: out_hits + r * hit_cap, out_hit_counts + r --: classify per tile of
 *        1 024 LINES (2 * k_lists wave-wide searches bound the lists' slices inside the tile, so a list of 10^6 entries costs
 *        what any other costs), the one-block scan of pire_hip_select, scatter; no atomics, no block waits for another: the
 *        same input gives the same bytes.  Scratch (n / 8 + n / 256 bytes, and n bytes more where out_hit_members is asked
 *        for) comes from the stream-ordered allocator: the rule and the capture-mode caveat stated at pire_hip_select.  The
 *        lists and out_hit_members may have any alignment.  A list that is not ascending, or that names lines >= n, gives an
 *        unspecified selection; even then the call reads nothing outside lists[j][0, k_j) and writes nothing outside what is
 *        stated above.  Otherwise host pointers: staged, synchronises, the lists come back only as far as they were written;
 *        a list that is not strictly ascending or that names a line >= n is PIRE_HIP_EINVAL, and nothing is written.
 * PIRE_HIP_EINVAL before any device is touched: k_lists == 0 or > PIRE_HIP_COMBINE_MAX_LISTS; null lists or list_caps;
 * list_caps[j] > 0 with null lists[j]; null out_hit_count; hit_cap > 0 with null out_hits; out_hit_members without out_hits;
 * n >= 2^32; a list_caps[j] >= 2^32.
 * pire_hip_last_kernel() is not changed by the pass.  No first-use self-test: it takes no table (as pire_hip_context).
 * The result is a hit list like any other: it chains into pire_hip_context, pire_hip_files, pire_hip_gather and into
 * pire_hip_combine again.
 */
#define PIRE_HIP_COMBINE_MAX_LISTS 6u
int pire_hip_combine(const uint64_t* const* lists, const uint64_t* const* list_counts, const uint64_t* list_caps,
                     uint32_t k_lists, uint64_t n, uint64_t truth, uint32_t flags,
                     uint64_t* out_hits, uint8_t* out_hit_members, uint64_t hit_cap, uint64_t* out_hit_count, void* stream);

/*
 * Raw bytes in, the lines that a boolean function of up to six scans selects out, behind one call, one split and one wait:
 * `grep a | grep -v b`, `awk -F'\t' '$3 ~ /a/ && $5 !~ /b/'`, a Scanner term and a SlowScanner term on the same lines.
 * terms[k_terms] is a HOST array in both flag modes.  Term j scans the whole line (column == PIRE_HIP_TERM_LINE) or the
 * field `column` of it, cut as pire_hip_fields cuts it with sep and field_mode (one cut per distinct column, sep and
 * field_mode), with its own run_flags (PIRE_HIP_RUN_BEGIN | _END | _GENERIC):
 *   table       the lines pire_hip_run_select lists under `want` (NULL: Final; host or device memory like the call's other
 *               pointers, pire_hip_table_mask_words(table) words)
 *   slow_table  the lines pire_hip_slow_run_select lists under `mode` (0, or PIRE_HIP_FINAL_SELECT_ZERO: the lines it does
 *               NOT match)
 * exactly one of the two per term.  The k_terms lists live in stream-ordered scratch (8 bytes a line a term at most);
 * pire_hip_combine with `truth` (bit j of the member mask: term j) gives out_hits, out_hit_members, hit_cap and
 * *out_hit_count, as stated there.  out_hit_spans[hit_cap][2] (nullable, needs out_hits): the whole line of out_hits[r] as a
 * byte range of raw, delimiter not included.  out_term_counts[k_terms] (nullable): the number of lines of every term's own
 * list (`grep -c` of every term).  *out_line_count, raw, size, delim, the one synchronisation of `stream` EVEN WITH
 * PIRE_HIP_RUN_ON_DEVICE and the refusal of 2^32 lines: as pire_hip_run_lines_select.  flags carries
 * PIRE_HIP_RUN_ON_DEVICE and nothing else.
 * The gather form: out_hits is nullable (the list then lives in scratch of the library's own); tail, out_text, text_cap,
 * out_offsets (hit_cap + 1 entries), out_bytes: as pire_hip_gather_spans.
 * PIRE_HIP_EINVAL before any device is touched: null terms, k_terms == 0 or > PIRE_HIP_COMBINE_MAX_LISTS; a term with both
 * tables or neither; a slow term with a mode above PIRE_HIP_FINAL_SELECT_ZERO; a column term with sep > 255, sep == delim or
 * unknown bits in field_mode; bits in flags other than PIRE_HIP_RUN_ON_DEVICE; what pire_hip_split refuses of raw, size and
 * delim; what pire_hip_combine refuses of its outputs; out_hit_spans without out_hits; the gather form: what
 * pire_hip_gather_spans refuses of its outputs.  Host pointers with size == 0: zeros (out_term_counts all zero,
 * out_offsets[0] = 0 where not null), no device is touched.
 */
#define PIRE_HIP_TERM_LINE (~0u)
typedef struct pire_hip_line_term {
    pire_hip_table* table;            /* exactly one of table / slow_table */
    pire_hip_slow_table* slow_table;
    const uint64_t* want;             /* table terms: as pire_hip_select (NULL: Final); host or device like the call's other pointers */
    uint32_t mode;                    /* slow terms: 0 or PIRE_HIP_FINAL_SELECT_ZERO */
    uint32_t run_flags;               /* PIRE_HIP_RUN_BEGIN | _END | _GENERIC */
    uint32_t column;                  /* PIRE_HIP_TERM_LINE: the whole line; else the field, as pire_hip_fields */
    uint32_t sep, field_mode;         /* as pire_hip_fields; ignored for PIRE_HIP_TERM_LINE */
} pire_hip_line_term;
int pire_hip_lines_combine_select(const pire_hip_line_term* terms, uint32_t k_terms, uint64_t truth,
                                  const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint64_t* out_line_count,
                                  uint64_t* out_hits, uint64_t* out_hit_spans, uint8_t* out_hit_members, uint64_t hit_cap,
                                  uint64_t* out_hit_count, uint64_t* out_term_counts, void* stream);
int pire_hip_lines_combine_gather(const pire_hip_line_term* terms, uint32_t k_terms, uint64_t truth,
                                  const void* raw, uint64_t size, uint32_t delim, uint32_t flags, uint64_t* out_line_count,
                                  uint64_t* out_hits, uint64_t* out_hit_spans, uint8_t* out_hit_members, uint64_t hit_cap,
                                  uint64_t* out_hit_count, uint64_t* out_term_counts,
                                  uint32_t tail, void* out_text, uint64_t text_cap, uint64_t* out_offsets, uint64_t* out_bytes,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIRE_HIP_H */
