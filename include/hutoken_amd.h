/*
 * hutoken_amd.h -- C ABI of the MI355X-native batch BPE encode path.
 *
 * This is the drop-in boundary for huToken's encode direction.  Each entry point
 * names the reference interface it replaces (paths are into the reference tree,
 * matyasosvath/hutoken @ 2025-09-05).  Plain pointers and sizes only; no Python,
 * torch or HIP types appear in a signature (a HIP stream is passed as void*).
 * INTEGRATION.md shows the binding a maintainer would add to src/lib.c.
 *
 * All results are bit-exact with the reference's string-keyed path
 * (src/core.c:66-209, 339-511) on the same inputs.  There is no CPU fallback:
 * every encode call runs on the GPU or fails with HUTK_E_DEVICE.
 */
#ifndef HUTOKEN_AMD_H
#define HUTOKEN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hutk_ctx hutk_ctx;

/* return codes; the comment names the Python exception the reference raises in
 * the same situation (src/lib.c) */
enum {
    HUTK_OK = 0,
    HUTK_E_FILE_NOT_FOUND = 1,  /* FileNotFoundError (lib.c:243-250, 460-469) */
    HUTK_E_VALUE = 2,           /* ValueError        (lib.c:295-388, 487-543) */
    HUTK_E_MEMORY = 3,          /* MemoryError */
    HUTK_E_ARG = 4,             /* TypeError / bad argument */
    HUTK_E_DEVICE = 5,          /* no GPU, HIP failure: the path fails loudly */
    HUTK_E_UNSUPPORTED = 6,     /* a file shape the device tables cannot hold */
    HUTK_E_CAPACITY = 7,        /* ids_cap below hutk_ids_capacity() */
    HUTK_E_NUL_BYTE = 8,        /* a 0x00 byte inside a document */
    HUTK_E_WORD_TOO_LARGE = 9,  /* device-side note only, see HUTK_DOC_WORD_TOO_LARGE */
    HUTK_E_INVALID_UTF8 = 10    /* non-byte-encoder mode only; the reference's
                                   behaviour there is undefined */
};

/* per-document status values written to status[] */
enum {
    HUTK_DOC_OK = 0,
    HUTK_DOC_WORD_TOO_LARGE = 1, /* a word longer than 262144 bytes (core.c:402-407).  The
                                    reference reports NOTHING for it (core.c:503 clears the
                                    message again) and ends the document there; so does
                                    hutk_encode_batch: the ids are those before that word */
    HUTK_DOC_INVALID_UTF8 = 2,
    /* decode direction */
    HUTK_DOC_ID_OUT_OF_RANGE = 3, /* an id < 0 or >= the number of vocabulary lines (src/core.c:523-531) */
    HUTK_DOC_ID_UNDECODABLE = 4,  /* an id without a unique key, or a token whose decoding depends on its
                                     neighbours (see hutk_decode_batch) */
    /* token spans */
    HUTK_DOC_SPAN_MISMATCH = 5    /* the document's text does not hold a token's decoded bytes where the token's
                                     span lies (see hutk_token_spans_device): its spans are unspecified */
};

/* Replaces _hutoken.initialize(vocab_file_path, special_file_path, prefix,
 * is_byte_encoder, ...) for the encode direction: src/lib.c:185-571
 * (initialize_context 128-183, vocab loader 243-388, special-character loader
 * 460-571) and struct EncodeContext (include/hutoken/taskqueue.h:16-25).
 * The decode tables are built alongside (hutk_decode_*), the regex pattern is set with
 * hutk_ctx_set_pattern.  `device` is a HIP device ordinal, or -1 for the current
 * device.  On failure *out is NULL and hutk_last_error() holds the message. */
int hutk_ctx_create(hutk_ctx** out, const char* vocab_path, const char* special_path,
                    const char* prefix, int is_byte_encoder, int device);

/* The same with _hutoken.initialize's `merges_file_path` (src/lib.c:573-663): when
 * the file holds at least one countable line the context encodes with the
 * reference's ID-KEYED merge loop (bpe_encode_arena_ids, src/core.c:211-337; unit
 * split and id lookup of src/core.c:457-477): rank = line order among the rules
 * whose left, right and concatenation are vocabulary keys, result = the id of the
 * concatenation, a repeated (left id, right id) keeps its last rule.  A file with
 * no countable line (empty, comments only) leaves the string-keyed path in force,
 * as in the reference.  merges_path == NULL is hutk_ctx_create.  A special-character
 * replacement of more than one character is several units per input item on this path
 * (src/core.c:460-474 splits it per character): accepted, its words take the exception path. */
int hutk_ctx_create_merges(hutk_ctx** out, const char* vocab_path, const char* special_path,
                           const char* prefix, int is_byte_encoder, const char* merges_path,
                           int device);

/* _hutoken.initialize's `pattern` (src/lib.c:188-205, 229-232): the regex pre-token path of encode(), src/core.c:350-360,
 * 372-378, 392-400, 498-500.  `pattern` is a POSIX extended regular expression; the words of a document are the
 * successive LEFTMOST matches at or after a cursor, text between them is dropped, an empty match moves the cursor one
 * byte on.  Matching is libc's regcomp/regexec in the process's locale, exactly the calls the reference makes, run on
 * the host by hutk_encode_batch / hutk_encode (one compiled pattern per host thread); pretokenizer and merge loop stay
 * on the GPU.  NULL returns to the hand-written splitter (src/parser.c).  HUTK_E_VALUE: the pattern does not compile
 * (the reference compares regcomp()'s result with `true` and goes on with an uncompiled pattern for every other error
 * code).  A context with a prefix keeps it: the prefix goes with a document's first match (src/core.c:364-366, 421-451).
 * hutk_encode_batch_device on a context with a pattern copies the bytes down for regexec and SYNCHRONISES with the
 * stream (the only form of the call that does); the encode itself stays on the device buffers. */
int hutk_ctx_set_pattern(hutk_ctx* ctx, const char* pattern);

/* Several GPUs behind ONE context of one process (`device_mask`).  The reference's
 * batch_encode spreads the documents of a batch over host threads, balanced by a DP on their lengths
 * (src/lib.c:779-794, 48-57); here hutk_encode_batch cuts a batch of at least 4 MiB (HUTK_MULTI_MIN_BYTES overrides) into
 * runs of whole documents with about the same number of bytes, one per device, encodes them side by side on a host
 * thread each, and puts the ids together in document order: ids, offsets and status are those of one device.
 * hutk_ctx_add_device adds `device` (an ordinal of this process; the same ordinal may be added again) with the tables
 * the context was created from; everything that takes device pointers (hutk_encode_batch_device,
 * hutk_decode_batch_device) and the decode direction stay on the context's first device. */
int hutk_ctx_add_device(hutk_ctx* ctx, int device);
int hutk_ctx_device_count(const hutk_ctx* ctx); /* 1 + the devices added; 0 for a host-only context */

/* The reference never frees its contexts (lib.c:129-155); this one can be. */
void hutk_ctx_destroy(hutk_ctx* ctx);

/* Message of the last failure on this thread (static storage, never NULL). */
const char* hutk_last_error(void);

/* Worst-case number of ids for a batch of n_bytes bytes in n_docs documents
 * (#ids <= #units <= bytes x the most units one input item can become + prefix units per document).
 * DEVICE MEMORY: beside the caller's buffers a context keeps a workspace that grows to the largest batch it has seen --
 * about 18 bytes per input byte for ordinary vocabulary files.  A special-characters file with a replacement of SEVERAL
 * units (a Llama-style "<0x0A>" on the merges path, test_pretokenizer.c:38-41's 'a' -> "Alpha") makes every word that
 * holds such an item an exception word: the exception arrays are then sized for a word per byte and for that many units
 * per byte, about 60 + 12 x (units per item) bytes of workspace per input byte (a 500 MB batch: tens of GB).  Cut such
 * batches smaller; hutk_encode_batch does so by itself (HUTK_PIPE_CHUNK_MB). */
int64_t hutk_ids_capacity(const hutk_ctx* ctx, int64_t n_bytes, int64_t n_docs);

/* Replaces the worker pool of p_batch_encode, src/lib.c:779-794, i.e. N threads
 * calling `void encode(struct EncodeTask*)` (include/hutoken/core.h:11,
 * src/core.c:339-511) once per document.  Batch-granular: documents are packed
 * back to back in `bytes`; document i is bytes[offsets[i] .. offsets[i+1]).
 * Host buffers in, host buffers out (the copies over PCIe are inside the call).
 *   ids_out      int32[ids_cap], ids_cap >= hutk_ids_capacity(...)
 *   out_offsets  int64[n_docs+1]; document i's ids are
 *                ids_out[out_offsets[i] .. out_offsets[i+1])
 *   status       int32[n_docs] (HUTK_DOC_*), may be NULL
 * Returns HUTK_OK or the first error. */
int hutk_encode_batch(hutk_ctx* ctx, const uint8_t* bytes, const int64_t* offsets,
                      int64_t n_docs, int32_t* ids_out, int64_t ids_cap,
                      int64_t* out_offsets, int32_t* status);

/* THREADS AND STREAMS.  A context owns one workspace (tile metadata, symbol runs, exception lists), so the calls on one
 * context are serialised: on the host by a mutex inside the context (any thread may call), on the device by an event --
 * each asynchronous call records it behind its last kernel and the next call makes its stream wait for it before its
 * first kernel, whichever streams the two calls use.  Nothing races and nothing is freed under a running kernel, but two
 * calls on ONE context do not overlap; give every stream that should encode concurrently a context of its own (the
 * tables are a few MB).  The reference's contexts are read-only and shared by its worker threads (taskqueue.h:16-25); its
 * concurrency is inside one batch_encode call, as is this library's. */

/* Same computation with every buffer already resident in device memory (the
 * form bench.py times and a GPU data loader would call).  n_bytes must equal
 * offsets[n_docs] (the host needs it to size the launch without a sync).
 * Work is enqueued on `hip_stream` (a hipStream_t, NULL = default stream) and
 * the call returns without synchronising (a context with a regex pattern excepted:
 * hutk_ctx_set_pattern); d_err receives the first device-side
 * error code (HUTK_OK when none) and may be NULL.  d_bytes must be 16-byte
 * aligned.  A document with a word of more than 262144 bytes ends in front of that
 * word, as the reference's does (src/core.c:402-407, 503): d_status[i] =
 * HUTK_DOC_WORD_TOO_LARGE, *d_err = HUTK_E_WORD_TOO_LARGE (a note, not a failure),
 * and d_out_offsets / d_ids_out hold the shortened document -- the same as
 * hutk_encode_batch returns. */
int hutk_encode_batch_device(hutk_ctx* ctx, const uint8_t* d_bytes, const int64_t* d_offsets,
                             int64_t n_docs, int64_t n_bytes, int32_t* d_ids_out,
                             int64_t ids_cap, int64_t* d_out_offsets, int32_t* d_status,
                             int32_t* d_err, void* hip_stream);

/* Page-locked host memory for the buffers handed to hutk_encode_batch: with it the chunked
 * path of hutk_encode_batch copies by DMA while the previous chunk is being encoded and the one
 * before is being copied back (pageable buffers work too, at roughly a third of the rate).
 * The pages are taken from the current HIP device's NUMA node where the host has several, provided the calling thread
 * runs under the default memory policy (a policy given with numactl --membind / --interleave is the caller's and stays;
 * HUTK_HOST_ALLOC_NUMA=0: the policy is never touched).  The reference has no counterpart (it strdup()s every text, src/lib.c:770-772). */
void* hutk_host_alloc(size_t n_bytes);
void hutk_host_free(void* p);

/* Replaces p_encode, src/lib.c:668-720 (one document on the calling thread). */
int hutk_encode(hutk_ctx* ctx, const uint8_t* text, int64_t len, int32_t* ids_out,
                int64_t ids_cap, int64_t* n_ids, int32_t* status);

/* Decode direction.  Replaces the worker pool of p_batch_decode / p_decode (src/lib.c:876-1126): one
 * decode(struct DecodeTask*) per document (src/core.c:513-581: token strings concatenated, then
 * pretokenizer_decode, src/pretokenizer.c:197-296: prefix stripped from the front, special values mapped
 * back to their bytes by longest match, other characters to the byte of their code point (byte-encoder
 * mode, '?' above 255) or copied).
 * ids[id_offsets[d] .. id_offsets[d+1]) are the tokens of document d; the decoded BYTES of document d are
 * bytes_out[out_offsets[d] .. out_offsets[d+1]) (the Python layer cuts at the first 0x00 and decodes UTF-8
 * like PyUnicode_FromString, lib.c:938-939).  bytes_out == NULL: only out_offsets (hence the sizes) and
 * status are produced; call again with out_offsets[n_docs] bytes of room.
 * Returns HUTK_E_VALUE when an id is out of range (the reference's ValueError "Element must be
 * non-negative and less than vocab size.") and HUTK_E_UNSUPPORTED when a token cannot be decoded on its
 * own: an id that no key or several keys carry (uninitialised memory / hash-map order in the reference),
 * or a token that ends inside a longer special value or inside a character (its decoding would depend
 * on the next token).  status[] names the documents. */
int hutk_decode_batch(hutk_ctx* ctx, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs,
                      uint8_t* bytes_out, int64_t bytes_cap, int64_t* out_offsets, int32_t* status);
/* The same on device-resident buffers, asynchronously on `hip_stream`; *d_err receives the error code
 * (HUTK_E_VALUE, HUTK_E_UNSUPPORTED, or HUTK_E_CAPACITY when the text does not fit bytes_cap: nothing is written at or
 * beyond d_bytes_out + bytes_cap, out_offsets and status are complete all the same), d_status[] (may be NULL) the
 * documents with a bad id.  A bad id contributes no bytes; the other tokens and documents are decoded as ever.
 * Alignment: that of the element types is enough.  d_bytes_out may start at ANY byte address (the 16-byte stores are
 * aligned on the address written to, the bytes around the output are left alone); d_ids needs 4 bytes (16 take the
 * faster loads).  d_ids may be NULL when n_ids == 0, d_bytes_out == NULL asks for out_offsets and status only.
 * Token length: every decoded length the loader accepts (vocabulary keys of up to 2047 bytes) is decoded exactly,
 * whatever a tile of 2048 tokens adds up to. */
int hutk_decode_batch_device(hutk_ctx* ctx, const int32_t* d_ids, const int64_t* d_id_offsets,
                             int64_t n_docs, int64_t n_ids, uint8_t* d_bytes_out, int64_t bytes_cap,
                             int64_t* d_out_offsets, int32_t* d_status, int32_t* d_err, void* hip_stream);

/* Introspection (tests, bench). */
int64_t hutk_vocab_size(const hutk_ctx* ctx);      /* distinct keys loaded */
int64_t hutk_pair_table_entries(const hutk_ctx* ctx);
int hutk_uses_merges(const hutk_ctx* ctx);         /* 1: the id-keyed merge path is in force */
int hutk_device_ordinal(const hutk_ctx* ctx);
/* out8: distinct keys, vocabulary symbols, symbols, pair entries, pair slots,
 * rank_is_sym, ident_ids, whole-word table entries.  Passing device = -2 to hutk_ctx_create
 * builds a host-only context (tables, no GPU) for this kind of inspection;
 * encode calls on it fail with HUTK_E_DEVICE. */
int hutk_table_stats(const hutk_ctx* ctx, int64_t* out8);

/* The learned table of multi-token words.  A byte-encoder context whose symbols fit 16 bits and whose ids rise with
 * the merge order keeps, on its device, the ids of the words its merge loop has encoded (2 .. 30 bytes, up to 16 ids);
 * a later occurrence of the same bytes, in this call or any later one, takes them from the table.  Batches of more
 * than 32 tiles fill it; every batch reads it.  Results are the same with and without it.  It never evicts: once three
 * quarters of its slots are in use, or a batch's words mostly find their buckets full, it stops learning until it is
 * cleared.
 * Environment, read when the context is created: HUTK_WORD_CACHE=0 no table; HUTK_WORD_CACHE_LOG2=k 2^k buckets of two
 * slots (default 19: 64 MiB).
 * out4: entries, capacity in slots (0: this context has no table), candidates the last learning batch handed to the
 * table, 1 while it learns.  Both calls wait for the context's last asynchronous call; clear empties the table and
 * lets it learn again. */
int hutk_ctx_word_cache_stats(hutk_ctx* ctx, int64_t* out4);
int hutk_ctx_word_cache_clear(hutk_ctx* ctx);

/* Device time of the most recent hutk_encode_batch_device/hutk_encode_batch call,
 * from HIP events recorded on the launch stream: the dominant kernel
 * ("encode tiles") and the whole enqueue.  Synchronises on those events. */
int hutk_last_timing(hutk_ctx* ctx, float* ms_tile_kernel, float* ms_total);

/* Diagnostic: pairs of the (left, right) -> merged table that live in their second bucket (a lookup for them
 * costs two loads instead of one). */
int64_t hutk_debug_pairs_second(const hutk_ctx* ctx);

/* Diagnostic: entries of the whole-word table's companion for words of 15..28 bytes (13..28 with 32-bit symbols). */
int64_t hutk_debug_long_words(const hutk_ctx* ctx);

/* Diagnostic: the seam map the tile kernel splits words by.  Bit (y - 0xE0) of out256[x] is set when some merge of
 * this vocabulary can join a token that ends with input byte x to one that begins with input byte y (0xE0..0xFF, the
 * lead bytes of three- and four-byte characters); where it is clear the reference's merge loop (src/core.c:66-209,
 * 211-337) can never produce a token across x | y, and the word is encoded as two.  Returns 1 when the map is in
 * use, 0 when it is switched off (HUTK_NO_SEAM=1). */
int hutk_debug_seam(const hutk_ctx* ctx, uint32_t* out256);
/* Diagnostic: the seam map's second level (vocabularies whose merges cover every (last byte, lead byte) pair but join only
 * some pairs of whole characters).  a3, b3: the three bytes of the character in front of a boundary and of the one behind
 * it, little-endian.  Returns 1 when no token can span a3 | b3 -- the tile kernel starts a word at b3 although the first
 * level says "may join" -- and 0 otherwise (also when the level is off).  tests/test_seam_cpu.py. */
int hutk_debug_seam2_cut(const hutk_ctx* ctx, uint32_t a3, uint32_t b3);
/* Diagnostic, host only (nothing is launched): which tile kernel a plain batch (no regex pattern) of n_bytes would be
 * given by hutk_encode_batch_device under the environment of this moment (HUTK_PTILES, HUTK_PTILES_MIN_TILES; the seam
 * switch as the context read it when it was created).  0: the ordinary tile kernel.  1: the persistent one.  2: both are
 * enqueued and a sample of the batch's bytes decides on the device.  -1: bad argument.  The encode enqueues by the same
 * function, so a test that means to reach one of the kernels can assert that it does.  A host-only context answers from
 * its tables.  tests/test_gpu_ptiles_edges.py. */
int hutk_debug_tile_kernel(const hutk_ctx* ctx, int64_t n_bytes);
/* Diagnostic: where the exception words (more than 32 units or 63 bytes, an end outside their tile's window, items of
 * several units) of the context's most recent encode went: hutk_encode_batch_device, or a host-form call, which reports
 * the last batch it enqueued.  The caller has synchronised that call's stream (the host forms have); nothing is launched,
 * the device's counters are copied once (the next encode zeroes them).  out8: exception records; the entries of the five
 * lists by length -- up to 128 units, up to 256, up to 512, up to 1024 (two, four, eight and sixteen lanes per word;
 * vocabularies without those routines leave them 0) and the words that get a wavefront each; the tail the host enqueued:
 * 0 = the exception, scan and finish kernels, 1 = the one-wavefront tail of a batch of at most 32 tiles and 4096
 * documents, 2 = none, the one-launch tile kernel of a host-form batch of at most four tiles did everything (no exception
 * word), 3 = the one-wavefront tail behind that one-launch kernel; 1 when the vocabulary has items of several units.  A
 * host-form batch that fell back from the one-launch kernel to the three launches reports 0 or 1.  A test that means to
 * reach one of the routines can assert that its batch did.  HUTK_E_ARG before the first encode.
 * tests/test_gpu_exc_kinds.py. */
int hutk_debug_exc_counts(const hutk_ctx* ctx, int64_t* out8);

/* Diagnostic build aid: clock64 stamps at the phase boundaries of the tile kernel.
 * hutk_debug_profile(ctx, 1), run a batch, then hutk_debug_profile_read returns the
 * mean shader cycles per phase over the first n_tiles tiles (out10[0] = their sum,
 * out10[k] = phase k).  Never enabled in timed runs. */
int hutk_debug_profile(hutk_ctx* ctx, int enable);
int hutk_debug_tile_bytes(void); /* input bytes per tile of the hot kernel */
int hutk_debug_profile_read(hutk_ctx* ctx, int64_t n_tiles, double* out10);
int hutk_debug_profile_raw(hutk_ctx* ctx, int64_t n_tiles, long long* out); /* the stamps, ten per tile */

/* Per-call profiling events cost a little; they are on by default. */
void hutk_set_timing(hutk_ctx* ctx, int enabled);

/* ---- training ------------------------------------------------------------------------------------------
 * BPE training on the GPU.  Replaces the reference's _hutoken.bpe_train / bbpe_train
 * (src/lib.c:76-126, src/bpe.c, src/bbpe.c) with the exact semantics of tools/train_vocab.cpp in "bytes" mode
 * (HUTK_TRAIN_BYTES) or "chars" mode (HUTK_TRAIN_CHARS):
 *   documents  bytes[offsets[i] .. offsets[i+1]); they may arrive over several hutk_trainer_add calls and the word
 *              counts accumulate.  A 0x00 byte inside a document fails the call with HUTK_E_NUL_BYTE and nothing
 *              of that call is counted.  Empty documents are allowed.
 *   words      the reference's splitter (src/parser.c, hutk_classify.h), never across documents, no length cap.
 *   symbols    bytes mode: byte values 0..255, A = 256.  chars mode: a unique word holding a byte < 0x20 or 0x7F is
 *              dropped; in the others each ' ' becomes E2 96 81 (U+2581), then the word is cut left to right into
 *              characters whose length comes from the lead byte (< 0x80: 1, 110xxxxx: 2, 1110xxxx: 3, any other: 4,
 *              cut short at the word's end; invalid UTF-8 is kept).  The distinct characters, sorted as byte strings,
 *              are the symbols 0..A-1.  Merge k (0-based) creates symbol A + k = bytes(a) + bytes(b).
 *   counts     pair (a, b): sum over unique words of word count x adjacent (a, b) positions (overlaps count),
 *              64-bit, integer atomics only: the result does not depend on the schedule.
 *   selection  highest count; ties go to the smaller (uint64)a << 32 | b; training stops after n_merges merges or
 *              when no pair has a count >= 1.
 *   merge      in every word, left to right and non-overlapping (aaaa -> n n, aaa -> n a).
 * hutk_trainer_create: device = HIP ordinal, -1 for the current device; bytes mode.
 * hutk_trainer_create_mode: the same with a mode (HUTK_TRAIN_BYTES or HUTK_TRAIN_CHARS; another value: HUTK_E_ARG).
 * hutk_trainer_alphabet: ends the adding phase (a later hutk_trainer_add returns HUTK_E_ARG), turns the unique words
 *   into symbols (once: later calls report the same) and writes the alphabet in id order: symbol i is
 *   bytes_out[offsets_out[i] .. offsets_out[i+1]), n_symbols + 1 offsets.  *n_symbols and *n_bytes (either may be
 *   NULL) receive the sizes; with bytes_out or offsets_out NULL only the sizes are reported; buffers too small for
 *   them return HUTK_E_CAPACITY.  Bytes mode: the 256 single bytes.  hutk_trainer_run calls it if it was not called.
 * hutk_trainer_run: may be called once per trainer (a second call returns HUTK_E_ARG); writes
 *   pairs_out[2k], pairs_out[2k+1] = (a, b) of merge k and counts_out[k] (optional) for k < *n_done.
 * hutk_trainer_stats: out8 = documents, bytes, word occurrences, unique words, symbols in unique words (bytes before
 *   the alphabet is made; characters of the kept words after that in chars mode), distinct pairs at the start, peak
 *   device workspace in bytes, microseconds of device time in the merge loop. */
#define HUTK_TRAIN_BYTES 0
#define HUTK_TRAIN_CHARS 1
typedef struct hutk_trainer hutk_trainer;
int hutk_trainer_create(hutk_trainer** out, int device);
int hutk_trainer_create_mode(hutk_trainer** out, int device, int mode);
int hutk_trainer_alphabet(hutk_trainer* t, uint8_t* bytes_out, int64_t bytes_cap, int64_t* offsets_out,
                          int64_t offsets_cap, int64_t* n_symbols, int64_t* n_bytes);
int hutk_trainer_add(hutk_trainer* t, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs);
int hutk_trainer_run(hutk_trainer* t, int32_t n_merges, int32_t* pairs_out, int64_t* counts_out, int32_t* n_done);
int hutk_trainer_stats(const hutk_trainer* t, int64_t* out8);
/* Which internal paths the trainer took (for tests; host-side values, no added synchronisation).  Writes the first
 * min(n, 13) of: pauses, pair-table rebuilds that grew it, that shrank it, all rebuilds, host synchronisations of the
 * merge loop, largest pair-table capacity, largest k_select grid, word-table rehashes, deferred word insertions,
 * largest number of deferred-insertion rounds in one add, words that moved from the long to the short list, unique
 * words dropped for a control byte (chars mode), character-set regrowths (chars mode). */
int hutk_trainer_debug_counters(const hutk_trainer* t, int64_t* out, int n);
void hutk_trainer_destroy(hutk_trainer* t);

/* ---- collation -----------------------------------------------------------------------------------------
 * From the ragged pair hutk_encode_batch_device writes (d_ids int32, d_offsets int64[n_docs + 1], offsets[0] == 0,
 * non-decreasing, offsets[n_docs] == n_ids) to what a model reads, on the GPU in one pass.  The reference has no
 * counterpart.  Ids are copied as they are, negative ones included.  bos_id / eos_id: HUTK_NO_TOKEN = not inserted; s is
 * the number of them present; the SEQUENCE of document i is [bos] ids_i [eos].  out_width 4 or 8: d_input_ids is int32
 * or int64.  All calls are asynchronous on hip_stream and never synchronise; *d_err (may be NULL) is cleared by the call and
 * receives HUTK_E_ARG when the kernel finds offsets[0] != 0, offsets[n_docs] != n_ids or offsets that point outside
 * the ids (nothing is read out of bounds; the outputs are then undefined).  No HIP device: HUTK_E_DEVICE, there is no CPU
 * fallback.  Sizes: n_docs < 2^31 - 1, max_len and seq_len < 2^31; element counts (n_docs x max_len, the stream) are 64-bit.
 *
 * PADDED.  Row i of d_input_ids[n_docs][max_len] is the sequence of document i; when it is longer than max_len the
 * document's own ids are cut to max_len - s (the first ones, or with HUTK_COLLATE_TRUNC_LEFT the last ones) and bos/eos
 * stay.  d_lengths[i] (may be NULL) is the sequence length after that; pad_id fills the rest of the row behind the
 * sequence, or with HUTK_COLLATE_PAD_LEFT in front of it; d_mask[n_docs][max_len] (may be NULL) is 1 on the sequence
 * and 0 on padding.  max_len < 1 or < s: HUTK_E_ARG.  n_docs == 0 writes nothing and succeeds.
 *
 * PACKED.  A packer holds a stream: the sequences of all documents added since it was created or last flushed, end to
 * end (an empty sequence -- no ids, s == 0 -- contributes nothing).  Row k is stream[k * seq_len .. (k + 1) * seq_len).
 * For the stream index p = k * seq_len + c inside the sequence that begins at b: position_ids[k][c] = p - max(b, k * seq_len)
 * (from 0 at every sequence start and every row start), segment_ids[k][c] = 1 + the number of sequences that begin in
 * (k * seq_len, p] (1, 2, 3 .. within a row; a sequence continued from the previous row is 1).  The rows depend on the
 * order of the documents only, not on how they were split over the add calls.
 *   the rows query  returns the number of rows the next add call with these sizes will write (-1: bad arguments).
 *   the add call    writes every complete row (n_rows receives their number, possibly 0) and keeps the remaining
 *                   < seq_len tokens, with their final position and segment values, in a device buffer of the packer.
 *                   rows_cap below the rows query: HUTK_E_CAPACITY, nothing is enqueued or consumed.
 *                   d_position_ids / d_segment_ids (int32) may be NULL.  After a call whose *d_err turned out non-zero
 *                   the packer's contents are undefined until it is flushed.
 *   the flush call  writes the kept tokens as one row padded with pad_id, position 0, segment 0 (*n_rows = 1), or
 *                   nothing when none are kept (*n_rows = 0), and empties the stream.
 *   pending         the number of tokens kept.
 * Calls on one packer are serialised like calls on one context: a mutex on the host, an event on the device.
 * Alignment, padded and packed alike (d_ids, d_input_ids, d_mask, d_lengths, d_position_ids, d_segment_ids): that of
 * the element type; 16 bytes gets the wide path. */
#define HUTK_COLLATE_TRUNC_LEFT 1
#define HUTK_COLLATE_PAD_LEFT 2
#define HUTK_NO_TOKEN INT32_MIN
int hutk_collate_padded_device(const int32_t* d_ids, const int64_t* d_offsets, int64_t n_docs, int64_t n_ids,
                               int64_t max_len, int32_t bos_id, int32_t eos_id, int32_t pad_id, int flags,
                               int out_width, void* d_input_ids, uint8_t* d_mask, int32_t* d_lengths, int32_t* d_err,
                               void* hip_stream);
typedef struct hutk_packer hutk_packer;
int hutk_packer_create(hutk_packer** out, int64_t seq_len, int32_t bos_id, int32_t eos_id, int32_t pad_id,
                       int out_width, int device);
int64_t hutk_packer_rows(const hutk_packer* p, int64_t n_docs, int64_t n_ids);
int hutk_packer_add_device(hutk_packer* p, const int32_t* d_ids, const int64_t* d_offsets, int64_t n_docs,
                           int64_t n_ids, void* d_input_ids, int32_t* d_position_ids, int32_t* d_segment_ids,
                           int64_t rows_cap, int64_t* n_rows, int32_t* d_err, void* hip_stream);
int hutk_packer_flush_device(hutk_packer* p, void* d_input_ids, int32_t* d_position_ids, int32_t* d_segment_ids,
                             int64_t* n_rows, void* hip_stream);
int64_t hutk_packer_pending(const hutk_packer* p);
void hutk_packer_destroy(hutk_packer* p);

/* PACKED CHANNELS.  A channel is a per-token array that lies along the same offsets as the ids: n_ids records of `per`
 * (1 or 2) elements of `width` (4 or 8) bytes -- the chat render's labels and turn ids, the [n_ids][2] of
 * hutk_token_spans_device, word ids.  A packer made by the create call below moves up to HUTK_PACKER_MAX_CHANNELS of them
 * along with the ids, so that channel c of every row element is, on top of the PACKED definition above:
 *   - for a stream position that holds document id number idx of the call, values_c[idx] (with per == 2 both elements of
 *     the record);
 *   - for a position the packer inserted (bos, eos) and for the padding of a flushed row, the channel's fill (an int64
 *     that must fit the width; with per == 2 it fills both elements);
 *   - carried tokens keep their channel values: the packer owns a carry per channel, two halves of seq_len * per
 *     elements of the channel's width, beside the carry of ids, positions and segments.
 * So the channel rows, like the id rows, depend on the order of the documents only, not on how they were split over the
 * add calls.  d_values and d_channel_rows are HOST arrays of n_channels DEVICE pointers: d_values[c] holds n_ids records,
 * d_channel_rows[c] receives [n_rows][seq_len] records (the flush call: one row).  With n_channels == 0 the create call
 * is hutk_packer_create and the two calls are the add and flush calls above.  On a packer that has channels those
 * older two return HUTK_E_ARG and consume nothing: they would lose the channels' carry.
 * The create call refuses, with HUTK_E_ARG and before any device call, n_channels outside 0 .. HUTK_PACKER_MAX_CHANNELS,
 * a width other than 4 or 8, a per other than 1 or 2 and a fill that does not fit its width.  A channel is read at the
 * index the id is read at, under the same range check: offsets that do not describe the ids set HUTK_E_ARG in *d_err
 * and nothing is read outside d_values[c][0 .. n_ids).  Alignment: that of the element; 16 bytes on every output gets
 * the wide path.
 *
 * Worked example: seq_len 4, eos 99, pad 0, documents [10,11,12], [], [20..25], [30], one channel equal to the ids, int64,
 * fill -100.  Three complete rows and the flushed one:
 *   ids        10 11 12 99   | 99 20 21 22     | 23 24 25 99     | 30 99 0 0
 *   segments   1 1 1 1       | 1 2 2 2         | 1 1 1 1         | 1 1 0 0
 *   channel    10 11 12 -100 | -100 20 21 22   | 23 24 25 -100   | 30 -100 -100 -100 */
#define HUTK_PACKER_MAX_CHANNELS 4
int hutk_packer_create_channels(hutk_packer** out, int64_t seq_len, int32_t bos_id, int32_t eos_id, int32_t pad_id,
                                int out_width, int device, int n_channels, const int* widths, const int* per,
                                const int64_t* fills);
int hutk_packer_channel_count(const hutk_packer* p);
int hutk_packer_add_channels_device(hutk_packer* p, const int32_t* d_ids, const int64_t* d_offsets, int64_t n_docs,
                                    int64_t n_ids, const void* const* d_values, void* d_input_ids,
                                    int32_t* d_position_ids, int32_t* d_segment_ids, void* const* d_channel_rows,
                                    int64_t rows_cap, int64_t* n_rows, int32_t* d_err, void* hip_stream);
int hutk_packer_flush_channels_device(hutk_packer* p, void* d_input_ids, int32_t* d_position_ids,
                                      int32_t* d_segment_ids, void* const* d_channel_rows, int64_t* n_rows,
                                      void* hip_stream);

/* PACKED ROWS FOR TRAINING.  Two passes over rows the packer wrote (from add, from flush, or both concatenated).
 *
 * The cu_seqlens call: d_segment_ids int32 [n_rows][L].  Flat element f = r * L + c starts a sequence when c == 0 or
 * seg[r][c] != seg[r][c - 1]; nothing else is looked at, so any int32 values are safe input.  (Segment numbers are dense
 * per row and 0 on padding: the sequences are the pieces of documents in each row, and a padding run is a sequence of
 * its own.)  d_cu_seqlens int32 [cap + 1] receives the rising starts, then n_rows * L in every remaining slot up to and
 * including slot cap: the surplus sequences have length zero.  d_info int32 [2] receives (n_seq, max_seqlen), max_seqlen
 * being the largest difference of two neighbouring entries of d_cu_seqlens.  cap < n_seq: HUTK_E_CAPACITY in *d_err, the
 * first cap starts are written (slot cap holds n_rows * L) and d_info[0] still holds the true n_seq.  n_rows * L >= 2^31:
 * HUTK_E_ARG, on the host and before anything else (the starts are int32: what varlen attention kernels take).
 * n_rows == 0: all zeros.  Never synchronises.  In the example above, the four rows and cap 8:
 * cu_seqlens = 0 4 5 8 12 14 16 16 16, info = (6, 4).
 *
 * The labels call: d_values [n_rows][L] of `width` 4 or 8 -- the input ids for plain causal LM, or a packed labels channel
 * whose columns off the loss are ignore_index already -- and d_segment_ids.  shift == 0: labels[r][c] = values[r][c]
 * where seg[r][c] != 0, ignore_index elsewhere.  shift != 0: labels[r][c] = values[r][c + 1] when c + 1 < L and
 * seg[r][c + 1] == seg[r][c] != 0, ignore_index elsewhere: no column predicts across a document boundary, a row end or
 * into padding.  d_labels has the width of d_values and must not overlap it or d_segment_ids; ignore_index must fit the
 * width.  In the example, ids and shift, i for ignore_index:  11 12 99 i | i 21 22 i | 24 25 99 i | 99 i i i.
 * hutk_debug_cu_tile: the elements a workgroup of the cu_seqlens count takes (tests place edges there). */
int hutk_packed_cu_seqlens_device(const int32_t* d_segment_ids, int64_t n_rows, int64_t seq_len, int64_t cap,
                                  int32_t* d_cu_seqlens, int32_t* d_info, int32_t* d_err, void* hip_stream);
int hutk_packed_labels_device(const void* d_values, int width, const int32_t* d_segment_ids, int64_t n_rows,
                              int64_t seq_len, int shift, int64_t ignore_index, void* d_labels, void* hip_stream);
int hutk_debug_cu_tile(void);

/* BEST FIT.  Rows of whole documents: only a sequence longer than a row is cut, and the pieces are packed
 * best-fit-decreasing (Ding et al. 2024, "Fewer Truncations Improve Language Modeling").  Inputs as above: d_ids int32,
 * d_offsets int64 [n_docs + 1]; L = seq_len; bos_id / eos_id / pad_id as for the packer, s the number of bos/eos given.
 * Document i has n_i ids; its sequence is [bos] ids [eos], m_i = n_i + s tokens.
 *   WHOLE ROWS.  A sequence is cut every L tokens: w_i = m_i div L whole rows and, when m_i mod L > 0, one ITEM of length
 *     l_i = m_i mod L, the sequence's tail.  m_i == 0 (an empty document, s == 0) gives nothing.  Output rows 0 .. W - 1,
 *     W = sum of w_i, are the whole rows in document order: segment 1, positions 0 .. L - 1.
 *   BINS.  The items are taken in the order (length descending, document number ascending).  Each goes into the open bin
 *     whose remaining room is the smallest that is still >= l; among bins of equal room into the lowest-numbered one; when
 *     none fits a new bin opens with room L.  The item's column is L - room before it is placed, its segment id the number
 *     of items already in the bin plus 1, its positions 0 .. l - 1 (the packer's rule: 0 at every document start and every
 *     row start).  Bin b is output row W + b.  Behind a bin's last item: pad_id, position 0, segment 0.
 *     n_rows = W + B.  The rows depend on the documents and their order only.
 * Outputs, R = rows_cap rows: d_input_ids [R][L] of out_width 4 or 8, d_position_ids and d_segment_ids int32 [R][L],
 * d_lengths int32 [R] (the filled columns), d_source int64 [R][L] (may be NULL): the index into d_ids of the token at that
 * element, -1 for bos, eos and padding.  Rows from n_rows up to R are all padding, length 0.
 * d_doc_map int64 [n_docs][4] = (whole_row, n_whole, row, col): the document's first whole row (-1 when n_whole == 0)
 * and where its item starts (-1, -1 when it has none).  d_info int64 [2] = (n_rows, W).
 *
 * Worked example: L 8, eos 99, pad 0, documents A = 10..14, B = [], C = 20..28, D = 30 31 32, E = 40, F = 50..56;
 * m = 6, 1, 10, 4, 2, 8.  Whole rows: C's first eight tokens (row 0), F with its eos (row 1).  Items in order: A 6, D 4,
 * C 2 (28 99), E 2, B 1.
 *   row 0   ids 20 21 22 23 24 25 26 27   segments 1 1 1 1 1 1 1 1   positions 0..7            length 8
 *   row 1   ids 50 51 52 53 54 55 56 99   segments 1 1 1 1 1 1 1 1   positions 0..7            length 8
 *   row 2   ids 10 11 12 13 14 99 28 99   segments 1 1 1 1 1 1 2 2   positions 0 1 2 3 4 5 0 1  length 8
 *   row 3   ids 30 31 32 99 40 99 99 0    segments 1 1 1 1 2 2 3 0   positions 0 1 2 3 0 1 0 0  length 7
 *   source of row 2: 0 1 2 3 4 -1 13 -1; of row 3: 14 15 16 -1 17 -1 -1 -1.
 *   doc_map: A (-1,0,2,0)  B (-1,0,3,6)  C (0,1,2,6)  D (-1,0,3,0)  E (-1,0,3,4)  F (1,1,-1,-1);  info = (4, 2).
 *
 * the rows bound  host only, no synchronisation: at least n_rows for any offsets that describe n_ids ids.  T = n_ids +
 *                 s * n_docs tokens in all.  Two bins are never both at most half full (the item that opened the later
 *                 one did not fit the earlier one), so all bins but one hold more than L / 2: B <= 2 * (T - W * L) / L + 1
 *                 and n_rows <= 2 * T div L + 1.  And W <= T div L, B <= n_docs.  The bound is the smaller of
 *                 2 * T div L + 1 and T div L + n_docs; 0 for n_docs == 0; -HUTK_E_ARG for bad arguments.
 * the plan call   documents -> d_doc_map, d_info.  rows_cap < n_rows: HUTK_E_CAPACITY in *d_err (d_info still holds the
 *                 true counts; the call itself writes nothing that rows_cap sizes).  Offsets that do not describe the ids:
 *                 HUTK_E_ARG in *d_err, the documents they name are taken as empty.  n_docs == 0: info = (0, 0).
 * the rows call   d_doc_map + ids -> the five row arrays, R = rows_cap rows, every element written exactly once.  It
 *                 trusts nothing: a doc_map row that is not what the offsets give (n_whole, whole_row), that points
 *                 outside the R rows or the row's columns, or that shares its place with another one, and offsets that
 *                 do not describe the ids, set HUTK_E_ARG in *d_err; what it cannot place is left out (the place
 *                 holds padding), and every write stays inside the outputs.  So after a plan that reported
 *                 HUTK_E_CAPACITY the rows call writes the rows below rows_cap and reports HUTK_E_ARG.  Items that
 *                 overlap without sharing their first column are not told apart from good ones: the later start wins.
 * the gather      d_out[e] = d_source[e] >= 0 ? d_values[d_source[e]] : fill over n elements: records of `per` (1 or 2)
 *                 elements of `width` (4 or 8) bytes, as the packer's channels -- labels, turn ids, spans, word ids --
 *                 along the source array of these rows, of the chat render or of fill-in-the-middle.  A source at or
 *                 above n_values: the fill, and HUTK_E_ARG in *d_err.  fill must fit the width.
 * All device calls are asynchronous on hip_stream.  Their scratch is one buffer per device that grows at a call larger
 * than any before it, and growing it waits for the device: the one synchronisation there can be.  The plan call makes the
 * buffer large enough for the rows call of rows_cap rows that follows it, so a pair of calls waits at most once, in front
 * of the plan, and a loop over batches of a steady size does not wait after its first pass.  Refused with HUTK_E_ARG before a device is looked for: seq_len < 1, < s, >= 2^31
 * or above 65536 (the length classes are ranked by 16 bits), negative counts, a width other than 4 or 8, a per other
 * than 1 or 2.  Alignment: that of the element; 16 bytes on every output (and L % 4 == 0) gets the wide path.
 * hutk_debug_bestfit_tile: the documents a workgroup of the plan's ranking pass owns at least, T = 4 wavefronts x 64.  A
 * wavefront owns a contiguous run of per_wave documents and walks it in chunks of 64: per_wave = 64 while n_docs <= 64 *
 * max(1, 2^21 div L), otherwise ceil(n_docs / max(1, 2^21 div L)) rounded up to a multiple of 64 (the rows call's
 * document passes: the same with 4096 wavefronts and runs of 128 at least).  Tests place edges at multiples of T / 4, T and per_wave. */
int64_t hutk_bestfit_rows_bound(int64_t n_docs, int64_t n_ids, int64_t seq_len, int s);
int hutk_bestfit_plan_device(const int64_t* d_offsets, int64_t n_docs, int64_t n_ids, int64_t seq_len, int32_t bos_id,
                             int32_t eos_id, int64_t rows_cap, int64_t* d_doc_map, int64_t* d_info, int32_t* d_err,
                             void* hip_stream);
int hutk_bestfit_rows_device(const int32_t* d_ids, const int64_t* d_offsets, const int64_t* d_doc_map, int64_t n_docs,
                             int64_t n_ids, int64_t seq_len, int32_t bos_id, int32_t eos_id, int32_t pad_id, int out_width,
                             int64_t rows_cap, void* d_input_ids, int32_t* d_position_ids, int32_t* d_segment_ids,
                             int32_t* d_lengths, int64_t* d_source, int32_t* d_err, void* hip_stream);
int hutk_rows_gather_source_device(const int64_t* d_source, int64_t n, const void* d_values, int64_t n_values, int width,
                                   int per, int64_t fill, void* d_out, int32_t* d_err, void* hip_stream);
int hutk_debug_bestfit_tile(void);

/* WINDOWS.  A long document becomes several overlapping rows instead of one truncated row (what other tokenizers call
 * stride with overflowing tokens, truncation on the right).  With C = max_len - s (the document ids a row holds) and
 * step = C - stride (0 <= stride < C), a document of n ids gives w(n) rows: 1 when n <= C (an empty document too),
 * 1 + ceil((n - C) / step) otherwise.  Row k of the document holds its ids [k * step, min(k * step + C, n)) as
 * [bos] ids [eos], padded with pad_id like a padded row; the last window is the short one.  The rows of document 0 come
 * first, then those of document 1, ..; d_row_offsets int64[n_docs + 1] is the exclusive prefix sum of w, strictly
 * increasing, d_row_offsets[n_docs] = n_rows.
 *   the rows bound  host only: n_docs + n_ids / step, at least n_rows for any offsets that describe n_ids ids; -HUTK_E_ARG
 *                   for sizes the other two calls refuse (s: the number of bos/eos tokens, 0 .. 2).
 *   the rows call   writes d_row_offsets[0 .. n_docs] in three launches (count, scan, write), so that the caller can read
 *                   n_rows and allocate.  *d_err receives HUTK_E_ARG for offsets[0] != 0, offsets[n_docs] != n_ids or a
 *                   document length below 0 or above n_ids (counted as 0 or n_ids; d_row_offsets is always written and
 *                   always strictly increasing).  The workgroup sums live in a small buffer per device that the first
 *                   call there allocates; calls that share it are serialised like calls on one packer.
 *   the fill call   writes d_input_ids[n_rows][max_len] and, where not NULL, d_mask[n_rows][max_len], d_lengths[n_rows]
 *                   (window ids + s) and d_row_map int64[n_rows][2] = {document, index of the row's first document id
 *                   inside the document = k * step}.  Element q of an unpadded row that is not bos or eos is
 *                   d_ids[d_offsets[document] + k * step + q - has_bos].  flags: HUTK_COLLATE_PAD_LEFT only.  *d_err
 *                   receives HUTK_E_ARG for offsets[0] != 0, offsets[n_docs] != n_ids, d_row_offsets[0] != 0 or
 *                   d_row_offsets[n_docs] != n_rows (nothing is written then), and for a document length or a
 *                   d_row_offsets entry that cannot be (such rows hold bos/eos and padding only).  Every index is
 *                   range-checked: nothing is read outside d_ids or the two offset arrays or written outside the n_rows
 *                   rows.  n_docs == 0 writes nothing and succeeds.
 * Refused with HUTK_E_ARG before a device is looked for: max_len < 1, < s + 1 or >= 2^31, stride < 0 or >= max_len - s,
 * an out_width other than 4 or 8, any flag but HUTK_COLLATE_PAD_LEFT, negative counts.  More than 2^31 - 1 workgroups in
 * the fill: HUTK_E_UNSUPPORTED. */
int64_t hutk_windows_rows_bound(int64_t n_docs, int64_t n_ids, int64_t max_len, int64_t stride, int s);
int hutk_windows_rows_device(const int64_t* d_offsets, int64_t n_docs, int64_t n_ids, int64_t max_len, int64_t stride,
                             int32_t bos_id, int32_t eos_id, int64_t* d_row_offsets, int32_t* d_err, void* hip_stream);
int hutk_collate_windows_device(const int32_t* d_ids, const int64_t* d_offsets, const int64_t* d_row_offsets,
                                int64_t n_docs, int64_t n_ids, int64_t n_rows, int64_t max_len, int64_t stride,
                                int32_t bos_id, int32_t eos_id, int32_t pad_id, int flags, int out_width,
                                void* d_input_ids, uint8_t* d_mask, int32_t* d_lengths, int64_t* d_row_map,
                                int32_t* d_err, void* hip_stream);

/* PAIRS.  Two texts in one row: row i is [bos] A' sep_ids B' [eos] of document i of two ragged pairs on one device,
 * (d_ids_a, d_offsets_a int64[n_pairs + 1]) and (d_ids_b, d_offsets_b).  Unlike the calls above, offsets_x[0] may be any
 * base: document i of side X is d_ids_x[offsets_x[i] .. offsets_x[i + 1]) and 0 <= offsets_x[0] <= .. <=
 * offsets_x[n_pairs] <= cap_x (the elements of d_ids_x) is what holds; both sides may share one ids buffer, and the
 * offsets need only their own 8-byte alignment.  sep_ids: a HOST array of n_sep = 0 .. HUTK_PAIR_MAX_SEP ids, none of
 * them HUTK_NO_TOKEN; s = [bos] + n_sep + [eos]; R = max_len - s >= 1 ids of room.  Both sides are cut on the right,
 * A' = A[0 .. ka), B' = B[0 .. kb); with na + nb <= R nothing is cut, otherwise by strategy
 *   HUTK_PAIR_LONGEST_FIRST  n1 <= n2 the shorter and longer length: n2 = n1 > R ? n1 : max(n1, R - n1); if still
 *                            n1 + n2 > R: n1 = R / 2, n2 = n1 + R % 2 (the longer side gets the odd id, on a tie B)
 *   HUTK_PAIR_ONLY_FIRST     kb = min(nb, R), ka = min(na, R - kb)
 *   HUTK_PAIR_ONLY_SECOND    ka = min(na, R), kb = min(nb, R - ka)    (the side not named is cut only when it alone
 *                            exceeds R)
 * d_token_types uint8[n_rows][max_len] (may be NULL) is 0 on bos, A' and every separator, 1 on B' and eos, 0 on padding;
 * d_lengths is ka + kb + s; d_mask and padding as in the padded rows.
 *   the fill, one row per pair   d_row_offsets == NULL and n_rows == n_pairs; any strategy; stride is checked and unused.
 *   the fill, windows            d_row_offsets from the rows call; HUTK_PAIR_ONLY_FIRST or _SECOND names the side that is
 *                   cut into windows (HUTK_PAIR_LONGEST_FIRST: HUTK_E_ARG).  The other side keeps ko = min(no, R) ids and
 *                   the cut side of n ids has C = R - ko ids of room per row: one row when n <= C or C == 0 (the cut
 *                   side is then empty), else step = max(1, C - stride) and 1 + ceil((n - C) / step) rows, row k holding
 *                   the cut side's ids [k * step, min(k * step + C, n)) with the whole kept side.  d_row_map
 *                   int64[n_rows][2] = {pair, k * step} (may be NULL; the one-row form writes {pair, 0}).
 *   the rows call   writes d_row_offsets int64[n_pairs + 1], the exclusive prefix sum of the pairs' row counts, always
 *                   strictly increasing, in three launches that share the windows' per-device buffer.
 *   the rows bound  host only: n_pairs + n_cut_ids (the ids of the cut side), at least n_rows for offsets that fit their
 *                   condition; -HUTK_E_ARG for sizes the other calls refuse (s: 0 .. 6).
 * *d_err receives HUTK_E_ARG for a document outside its condition (it counts as empty: its rows hold the other side,
 * the template's tokens and padding), and in the windows form for d_row_offsets[0] != 0 or d_row_offsets[n_pairs] !=
 * n_rows (nothing is written then) or an entry that is not the scan of the counts.  Every index is range-checked:
 * nothing is read outside the offsets or the ids or written outside the n_rows rows.  n_pairs == 0 writes nothing.
 * Refused with HUTK_E_ARG before a device is looked for: max_len < s + 1 or >= 2^31, stride < 0 or >= R, an unknown
 * strategy, n_sep outside 0 .. 4 or an absent id in sep_ids, an out_width other than 4 or 8, any flag but
 * HUTK_COLLATE_PAD_LEFT, negative counts. */
#define HUTK_PAIR_LONGEST_FIRST 0
#define HUTK_PAIR_ONLY_FIRST 1
#define HUTK_PAIR_ONLY_SECOND 2
#define HUTK_PAIR_MAX_SEP 4
int64_t hutk_pair_rows_bound(int64_t n_pairs, int64_t n_cut_ids, int64_t max_len, int64_t stride, int s);
int hutk_pair_rows_device(const int64_t* d_offsets_a, const int64_t* d_offsets_b, int64_t n_pairs, int64_t cap_a,
                          int64_t cap_b, int64_t max_len, int64_t stride, int strategy, int32_t bos_id,
                          const int32_t* sep_ids, int n_sep, int32_t eos_id, int64_t* d_row_offsets, int32_t* d_err,
                          void* hip_stream);
int hutk_collate_pairs_device(const int32_t* d_ids_a, const int64_t* d_offsets_a, const int32_t* d_ids_b,
                              const int64_t* d_offsets_b, const int64_t* d_row_offsets, int64_t n_pairs, int64_t cap_a,
                              int64_t cap_b, int64_t n_rows, int64_t max_len, int64_t stride, int strategy,
                              int32_t bos_id, const int32_t* sep_ids, int n_sep, int32_t eos_id, int32_t pad_id,
                              int flags, int out_width, void* d_input_ids, uint8_t* d_mask, uint8_t* d_token_types,
                              int32_t* d_lengths, int64_t* d_row_map, int32_t* d_err, void* hip_stream);

/* ---- chat: multi-turn conversations with assistant-only labels -----------------------------------------------
 * A render step between encode and collation.  The turns' contents are encoded as one document each by one encode
 * call; the render makes of them one sequence per conversation, a new ragged pair (d_out_ids, d_out_offsets) that
 * every layout above takes unchanged, plus per-token arrays ragged along the same offsets.  Inputs, on one device:
 *   d_ids int32, d_offsets int64[n_turns + 1]    the encode call's pair (offsets[0] == 0, offsets[n_turns] == n_ids)
 *   d_roles int32[n_turns]                       the role of every turn, 0 .. n_roles - 1
 *   d_conv_offsets int64[n_conv + 1]             into the turns: [0] == 0, non-decreasing, [n_conv] == n_turns
 * A TEMPLATE holds for each role r < n_roles <= HUTK_CHAT_MAX_ROLES a prefix and a suffix of 0 .. HUTK_CHAT_MAX_PART ids
 * each, suffix_loss[r] <= |suffix_r| (NULL: all of it), the number of leading suffix ids that carry loss, and bos_id /
 * eos_id (HUTK_NO_TOKEN = absent).  The sequence of conversation i with the turns t = co[i] .. co[i + 1] - 1 is
 *     [bos]  prefix[role_t] content_t suffix[role_t]  (for every t, in order)  tail
 * where tail is prefix[gen_role] with a generation prompt (gen_role >= 0), otherwise [eos]; asking for both is
 * HUTK_E_ARG.  A conversation without turns is [bos] tail.  With len(t) = |prefix| + n_t + |suffix| and T the exclusive
 * scan of len over all turns:
 *   d_turn_offsets int64[n_turns + 1] = T
 *   d_out_offsets[i] = T[co[i]] + i * fixed, fixed = [bos] + |tail|; n_out = d_out_offsets[n_conv]
 *   d_out_ids int32[n_out]     the sequences
 *   d_labels int32[n_out]      the id on the content and on the first suffix_loss[r] suffix ids of every turn whose
 *                              role's bit is set in loss_roles; ignore_index everywhere else: prefixes, the other
 *                              roles, bos, the generation prompt, eos
 *   d_turn_ids int32[n_out]    (may be NULL) the turn's index inside its conversation on the tokens of its prefix,
 *                              content and suffix, -1 on bos and tail
 *   d_src int64[n_out]         (may be NULL) the index into d_ids on content tokens, -1 elsewhere: what carries any
 *                              per-token array of the encode call (spans, word ids) over to the rendered stream
 *   the template    create copies the parts (HOST arrays: ids of all roles end to end, offsets int32[n_roles + 1]) into
 *                   a small table on `device` (-1: the current one), read-only afterwards: calls on one handle need
 *                   no serialisation among themselves.  destroy waits for the device first.  device == -2 keeps the
 *                   table on the host only, as a context's: the bound and every check below work, the two device calls
 *                   then end with HUTK_E_DEVICE.
 *   the ids bound   host only: n_ids + n_turns * max_r(|prefix_r| + |suffix_r|) + n_conv * fixed, at least n_out for any
 *                   roles; -HUTK_E_ARG for sizes the other calls refuse.
 *   the offsets call  writes d_turn_offsets (the rows scan of the windows: count, scan, write, sharing its per-device
 *                   buffer and its rule) and d_out_offsets (one launch).  *d_err receives HUTK_E_ARG for a role outside
 *                   [0, n_roles) or a turn length below 0 or above n_ids -- the turn then counts as rendered length 0,
 *                   it is left out and everything else is as stated -- and for d_offsets whose ends are not 0 and n_ids
 *                   or d_conv_offsets that do not rise from 0 to n_turns.  n_conv == 0 writes d_out_offsets[0] = 0.
 *   the render call writes the four per-token arrays.  *d_err receives HUTK_E_ARG for the above and for turn or out
 *                   offsets that are not what the offsets call writes; the outputs are then undefined, but nothing is
 *                   read outside the inputs or written outside out_cap elements (every index is range-checked).
 *                   n_out > out_cap: HUTK_E_CAPACITY in *d_err, and nothing is written at or behind out_cap.
 * All calls are asynchronous on hip_stream and never synchronise; *d_err (may be NULL) is cleared by each call.
 * Refused with HUTK_E_ARG before a device is looked for: n_roles outside 1 .. 16, a part longer than 32 ids or holding
 * HUTK_NO_TOKEN, part offsets that are not a scan from 0, suffix_loss[r] outside its suffix, a NULL template, gen_role
 * outside -1 .. n_roles - 1, gen_role >= 0 with an eos, loss_roles bits at or above n_roles, negative counts (n_conv
 * and n_turns: below 2^31 - 1), and with work to do (n_conv > 0) a NULL required buffer or one not aligned to its
 * element type.  16-byte alignment of an output gets it 16-byte stores. */
#define HUTK_CHAT_MAX_ROLES 16
#define HUTK_CHAT_MAX_PART 32
typedef struct hutk_chat_template hutk_chat_template;
int hutk_chat_template_create(hutk_chat_template** out, int device, int n_roles, const int32_t* prefix_ids,
                              const int32_t* prefix_offsets, const int32_t* suffix_ids, const int32_t* suffix_offsets,
                              const int32_t* suffix_loss, int32_t bos_id, int32_t eos_id);
void hutk_chat_template_destroy(hutk_chat_template* t);
int64_t hutk_chat_ids_bound(const hutk_chat_template* t, int64_t n_conv, int64_t n_turns, int64_t n_ids, int gen_role);
int hutk_chat_offsets_device(const hutk_chat_template* t, const int64_t* d_offsets, const int32_t* d_roles,
                             const int64_t* d_conv_offsets, int64_t n_conv, int64_t n_turns, int64_t n_ids, int gen_role,
                             int64_t* d_turn_offsets, int64_t* d_out_offsets, int32_t* d_err, void* hip_stream);
int hutk_chat_render_device(const hutk_chat_template* t, const int32_t* d_ids, const int64_t* d_offsets,
                            const int32_t* d_roles, const int64_t* d_conv_offsets, const int64_t* d_turn_offsets,
                            const int64_t* d_out_offsets, int64_t n_conv, int64_t n_turns, int64_t n_ids, int gen_role,
                            uint32_t loss_roles, int32_t ignore_index, int64_t out_cap, int32_t* d_out_ids,
                            int32_t* d_labels, int32_t* d_turn_ids, int64_t* d_src, int32_t* d_err, void* hip_stream);
int hutk_debug_chat_span(void);

/* ---- fill-in-the-middle (FIM): PSM and SPM, cut at tokens or at characters ----------------------------------------
 * A render step between encode and collation, of the chat render's shape: a document is cut into prefix / middle /
 * suffix and re-ordered behind three sentinel ids, so that a left-to-right model learns to infill (Bavarian et al. 2022).
 * A ragged pair (d_ids, d_offsets) goes in and a new ragged pair (d_out_ids, d_out_offsets) comes out, which every layout
 * above takes unchanged, plus per-token arrays along the same offsets.  THE RULE (csrc/hutk_fim.h holds it as code,
 * tests/fim_ref.py restates it in numpy):
 *   CONSTANTS.  The sentinels pre_id, suf_id, mid_id are required; end_id is optional (HUTK_NO_TOKEN = absent) and is
 *     appended behind the middle of transformed documents only; E = 1 with an end_id, else 0.  Kinds: 0 plain, 1 PSM,
 *     2 SPM.  Parts: 0 plain, 1 prefix, 2 middle, 3 suffix, 4 sentinel; loss_parts is a mask of 1 << part, and
 *     HUTK_FIM_LOSS_END (1 << 5) in it names the end sentinel alone, for loss on the middle and what closes it.
 *   DRAW.  Document number d = first_doc + i draws (u0, u1, u2, u3) = draw(seed, d, 0, DRAW_FIM) with DRAW_FIM = 4:
 *     Philox4x32-10 with key (low32(seed), high32(seed)) and counter (low32(d), high32(d), 0, 4) (csrc/hutk_philox.h).
 *     With len the document's length it is TRANSFORMED iff u0 < fim_below and 1 <= len < 2^31, and SPM iff transformed
 *     and u1 < spm_below, else PSM.  a = (uint64(u2) * (len + 1)) >> 32, b = (uint64(u3) * (len + 1)) >> 32,
 *     lo = min(a, b), hi = max(a, b), so 0 <= lo <= hi <= len.  The thresholds are integers in 0 .. 2^32, as in
 *     hutk_rows_mlm_device: a probability p is int(p * 2^32).  A plain document has lo = hi = len.
 *   TOKEN LEVEL.  len is the document's id count n.  With its ids x[0..n): prefix = x[0..lo), middle = x[lo..hi),
 *     suffix = x[hi..n); P = lo, M = hi - lo, S = n - hi.
 *       plain  x unchanged: n outputs of part 0.
 *       PSM    pre prefix suf suffix mid middle [end]: position 0 is pre, 1 .. P is x[p - 1], P + 1 is suf,
 *              P + 2 .. P + S + 1 is x[hi + p - P - 2], P + S + 2 is mid, the M positions behind it are x[lo + ..], the
 *              last is end.
 *       SPM    pre suf suffix mid prefix middle [end] (the paper's variant 2, what Megatron and bigcode call SPM):
 *              0 is pre, 1 is suf, 2 .. S + 1 is the suffix, S + 2 is mid, the P positions behind it are the prefix, the
 *              M positions behind those the middle, the last is end.
 *     A transformed document has n + 3 + E outputs, and d_out_offsets is the exclusive scan of the outputs.  Per token:
 *       d_out_ids int32   the id
 *       d_labels int32    (may be NULL) the id where loss_parts has the position's part (or HUTK_FIM_LOSS_END, on the
 *                         end sentinel), else ignore_index
 *       d_parts int32     (may be NULL) the part
 *       d_src int64       (may be NULL) the index into d_ids on document tokens, -1 on sentinels: the chat render's
 *                         source
 *     Example: x = 10 11 12 13 14, lo = 1, hi = 3, sentinels 1 / 2 / 3, end 4:
 *       PSM  1 10 2 13 14 3 11 12 4   source -1 0 -1 3 4 -1 1 2 -1
 *       SPM  1 2 13 14 3 10 11 12 4   source -1 -1 3 4 -1 0 1 2 -1
 *   CHARACTER LEVEL.  hutk_fim_cut_text_device cuts the packed text (d_bytes, d_offsets int64[n_docs + 1]) before it is
 *     encoded, so that no token straddles a cut.  len is the document's byte count; lo and hi come from the same draw;
 *     each cut then moves back to a UTF-8 character start: while 0 < pos < len, bytes[pos] is in 0x80 .. 0xBF and fewer
 *     than three steps were taken, pos -= 1.  It writes d_piece_offsets int64[3 n_docs + 1] -- the document's start,
 *     start + lo, start + hi for each document, then the end of the text -- and d_kinds int32[n_docs].  The bytes are not
 *     copied: the same d_bytes is encoded with the new offsets as 3 n_docs documents by ONE encode call.  A plain
 *     document is the pieces (whole, empty, empty), so its ids are those of the unsplit document.
 *     hutk_fim_plan_pieces_device then reads lo / hi / n of document i from the ids' offsets [3i .. 3i + 3] and the
 *     kind from d_kinds; it draws nothing.  The render is the same call as at token level.
 * The calls:
 *   the ids bound   host only: n_ids + (3 + E) * n_docs, at least n_out; -HUTK_E_ARG for sizes the other calls refuse.
 *   the text cut    one launch.  *d_err receives HUTK_E_ARG for offsets whose ends are not 0 and n_bytes or that
 *                   decrease; such a document counts as plain with length 0.  n_docs == 0 writes
 *                   d_piece_offsets[0] = 0 only (n_bytes must then be 0: HUTK_E_ARG otherwise).
 *   the plan calls  write d_out_offsets int64[n_docs + 1] (the rows scan of the windows: count, scan, write, sharing
 *                   its per-device buffer and its rule), d_plan int64[n_docs][4] = (src0, n, lo, hi) with src0 the
 *                   document's first id, and at token level d_kinds.  *d_err receives HUTK_E_ARG for offsets that do not
 *                   describe the ids and, from pieces, a kind outside 0 .. 2; such a document counts as plain with no
 *                   ids.  n_docs == 0 writes d_out_offsets[0] = 0 only.
 *   the render      writes the per-token arrays.  Nothing is trusted: *d_err receives HUTK_E_ARG for a plan row that is
 *                   not 0 <= lo <= hi <= n with src0 + n <= n_ids, a kind outside 0 .. 2, and d_out_offsets that are
 *                   not the scan of the rendered lengths; what does not fit leaves id 0, ignore_index, part -1,
 *                   source -1 at its place, and nothing is read outside the inputs.  n_out > out_cap: HUTK_E_CAPACITY
 *                   in *d_err, and nothing is written at or behind out_cap.
 * All device calls are asynchronous on hip_stream and never synchronise; *d_err (may be NULL) is cleared by each call.
 * Refused with HUTK_E_ARG before a device is looked for: negative counts, n_docs at or above 2^31 - 1, a negative
 * first_doc, thresholds outside 0 .. 2^32, a required sentinel equal to HUTK_NO_TOKEN, loss_parts with bits above
 * 1 << 5, a negative out_cap, and with work to do (n_docs > 0) a NULL required buffer or one not aligned to its element
 * type.  16-byte alignment of an output gets it 16-byte stores.  hutk_debug_fim_decide -> out3 = (kind, lo, hi) and
 * hutk_debug_fim_locate -> out2 = (part, the index inside the document or the sentinel's number 0 pre / 1 suf / 2 mid /
 * 3 end; part -1 for a p outside the document) are host only and call the two functions of csrc/hutk_fim.h. */
#define HUTK_FIM_PLAIN 0
#define HUTK_FIM_PSM 1
#define HUTK_FIM_SPM 2
#define HUTK_FIM_PART_PLAIN 0
#define HUTK_FIM_PART_PREFIX 1
#define HUTK_FIM_PART_MIDDLE 2
#define HUTK_FIM_PART_SUFFIX 3
#define HUTK_FIM_PART_SENTINEL 4
#define HUTK_FIM_LOSS_END 32
int64_t hutk_fim_ids_bound(int64_t n_docs, int64_t n_ids, int has_end);
int hutk_fim_cut_text_device(const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes, uint64_t seed,
                             int64_t first_doc, int64_t fim_below, int64_t spm_below, int64_t* d_piece_offsets,
                             int32_t* d_kinds, int32_t* d_err, void* hip_stream);
int hutk_fim_plan_tokens_device(const int64_t* d_offsets, int64_t n_docs, int64_t n_ids, uint64_t seed, int64_t first_doc,
                                int64_t fim_below, int64_t spm_below, int has_end, int64_t* d_out_offsets, int64_t* d_plan,
                                int32_t* d_kinds, int32_t* d_err, void* hip_stream);
int hutk_fim_plan_pieces_device(const int64_t* d_piece_id_offsets, const int32_t* d_kinds, int64_t n_docs, int64_t n_ids,
                                int has_end, int64_t* d_out_offsets, int64_t* d_plan, int32_t* d_err, void* hip_stream);
int hutk_fim_render_device(const int32_t* d_ids, const int64_t* d_plan, const int32_t* d_kinds, const int64_t* d_out_offsets,
                           int64_t n_docs, int64_t n_ids, int32_t pre_id, int32_t suf_id, int32_t mid_id, int32_t end_id,
                           uint32_t loss_parts, int32_t ignore_index, int64_t out_cap, int32_t* d_out_ids, int32_t* d_labels,
                           int32_t* d_parts, int64_t* d_src, int32_t* d_err, void* hip_stream);
int hutk_debug_fim_span(void);
int hutk_debug_fim_decide(uint64_t seed, int64_t doc, int64_t len, int64_t fim_below, int64_t spm_below, int64_t out3[3]);
int hutk_debug_fim_locate(int64_t n, int64_t lo, int64_t hi, int kind, int has_end, int64_t p, int64_t out2[2]);

/* ---- token spans (offset mapping) ----------------------------------------------------------------------
 * Which stretch of its document each id covers: from the packed text (d_bytes, d_offsets) and the ragged pair that
 * hutk_encode_batch_device wrote for it (d_ids, d_id_offsets; n_ids as in the collation calls: d_id_offsets[n_docs] ==
 * n_ids) to d_spans[n_ids][2] = {start, end}, half open, relative to the document's first byte; out_width 4 or 8: int32
 * or int64.  The reference has no counterpart.  An ITEM is what the pretokenizer consumes in one step
 * (src/pretokenizer.c:102-168): a byte with is_byte_encoder, otherwise a UTF-8 character whose length its lead byte
 * gives, cut short at the document's end.  Every id covers a whole number of consecutive items and the ids of a
 * document tile its encoded part from byte 0 on: a known id covers the items of its decoded text (what
 * hutk_decode_batch writes for it; for a document's first token the prefix-stripped form, so the tokens of a prefix that
 * was encoded as a word of its own get the empty span {0, 0}), an id of -1 (a unit the vocabulary does not hold,
 * core.c:205-207) covers the ONE item at the cursor.  A document cut at an over-long word has spans for the ids it has.
 *   unit  HUTK_SPANS_BYTES  start and end in bytes
 *         HUTK_SPANS_CHARS  in characters; a character starts at every byte b with (b & 0xC0) != 0x80.  end = the number
 *                           of character starts in doc[0, byte end); start of a non-empty span = the index of the
 *                           character that holds byte `byte start` (two byte-level tokens that split one character
 *                           both report it); an empty span is {c, c}, c = the character starts in front of it.
 * Nothing is taken on trust: the decoded bytes of every known id are compared with the source bytes of its span (and
 * the length of every -1 item with the pretokenizer's rule).  A difference -- ids that are not this text's, a special
 * value that equals an ordinary character, an id that cannot be decoded on its own -- sets status[doc] =
 * HUTK_DOC_SPAN_MISMATCH and *d_err = HUTK_E_UNSUPPORTED; that document's spans are then unspecified, every write stays
 * inside d_spans and the other documents are exact.
 * Refused at the call with HUTK_E_UNSUPPORTED: a context with a regex pattern (the text between matches is dropped),
 * a special-character replacement of several units, a special-character entry for a byte >= 0x80 without
 * is_byte_encoder.  Offsets that do not describe the buffers (negative, decreasing, beyond n_bytes or n_ids,
 * d_id_offsets[0] != 0, d_id_offsets[n_docs] != n_ids), or a document of 2^31 bytes or more with out_width 4: *d_err =
 * HUTK_E_ARG, nothing is read out of bounds, d_spans is not written.  n_docs == 0 or n_ids == 0 writes no span and
 * succeeds (with documents and no ids the offsets are still checked; d_ids and d_spans may then be NULL).  d_spans
 * need only be aligned to its element; 16-byte alignment gets 16-byte stores.  Also HUTK_E_UNSUPPORTED at the call: a
 * vocabulary with a token of 2 MiB or more.  Asynchronous on hip_stream (NULL: the context's stream), never synchronises once the context's workspace
 * has grown to the batch's size; serialised with the other calls on the context; runs on the context's first device.
 * d_status int32[n_docs] and d_err int32[1] may be NULL; both are cleared by the call.
 * hutk_token_spans: the same from host buffers (copies, calls the device form, waits); returns what *d_err held.
 * There is no CPU fallback. */
#define HUTK_SPANS_BYTES 0
#define HUTK_SPANS_CHARS 1
int hutk_token_spans_device(hutk_ctx* ctx, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                            int64_t n_bytes, const int32_t* d_ids, const int64_t* d_id_offsets, int64_t n_ids, int unit,
                            int out_width, void* d_spans, int32_t* d_status, int32_t* d_err, void* hip_stream);
int hutk_token_spans(hutk_ctx* ctx, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, const int32_t* ids,
                     const int64_t* id_offsets, int unit, int out_width, void* spans, int32_t* status);
/* For tests that size their batches by the kernels' own constants: the ids one workgroup takes, and the source bytes per
 * chunk of the rank structure over the character starts (64-byte blocks inside it). */
int hutk_debug_span_tile_ids(void);
int hutk_debug_span_chunk_bytes(void);

/* ---- special tokens --------------------------------------------------------------------------------------
 * Byte strings of the text that encode as ONE id each ("<|endoftext|>", chat-template markers), matched on the GPU.  The
 * reference has no counterpart: it parses a special_token_id argument and drops it, and its word splitter cuts such a
 * marker into pieces before any table is asked.  hutk_encode_batch, hutk_encode_batch_device and hutk_encode never look
 * at the set: they stay bit-exact with the reference.
 *
 * THE SET.  hutk_ctx_set_special_tokens installs n pairs (string i = bytes[offsets[i] .. offsets[i+1]), ids[i]) in place
 * of any earlier set; n == 0 removes it (the pointers may then be NULL).  HUTK_E_VALUE, and the set in force stays, for:
 * more than 1024 pairs, an empty string, a string of more than 255 bytes, a 0x00 byte, two equal strings, an id < 0.  An
 * id need not be a vocabulary line.  On a host-only context (device = -2) the call validates and builds the tables, no
 * more.  hutk_ctx_special_token_count: the pairs installed.
 *
 * MATCHING.  Inside one document, from left to right: at the cursor a special string matches when its bytes equal the
 * text there and it ends at or before the document's end (a match never spans two documents); of several that match at
 * one start the longest is taken, and if the longer ones fail the shorter one that matches; the cursor moves to the
 * match's end, else one byte on.  Leftmost first, then longest, never overlapping: "aa" on "aaaaa" matches at 0 and 2;
 * {"ab", "bc"} on "abc" takes "ab" and leaves "c" as text.
 *
 * ENCODING.  The matches cut a document into pieces: text, special, text, ..., text (text pieces may be empty).  Its ids
 * are, in order: for a text piece exactly what hutk_encode_batch_device returns for the piece AS A DOCUMENT OF ITS OWN --
 * so a context with a prefix gives every non-empty text piece its prefix (Hugging Face's "legacy" behaviour) -- and for a
 * special piece its one id.  No set installed, or no match in the batch: ids, offsets, status and *d_err are those of
 * hutk_encode_batch_device.  A DELIBERATE DIFFERENCE from "the document ends there": a text piece that holds a word of
 * more than 262144 bytes ends in front of that word, ONLY that piece; the pieces behind it are encoded as ever, the
 * document's status is HUTK_DOC_WORD_TOO_LARGE (the worst of its pieces') and *d_err the note HUTK_E_WORD_TOO_LARGE.
 *
 * hutk_special_ids_capacity: an upper bound on the ids of a batch.  Proof.  Let U = the most units an input item can
 * become and P = the prefix units a document can get, so that hutk_ids_capacity(b, d) = b U + d P + 1 bounds the ids of
 * any batch of b bytes in d documents.  With k matches the text pieces are n_docs + k documents of at most n_bytes - k
 * bytes together (a match covers at least one byte) and the special pieces give k ids:
 *     ids <= (n_bytes - k) U + (n_docs + k) P + k = n_bytes U + n_docs P + k (P + 1 - U),      0 <= k <= n_bytes.
 * For P + 1 <= U the maximum is at k = 0, otherwise at k = n_bytes; in both cases
 *     ids <= n_bytes max(U, P + 1) + n_docs P,
 * and the function returns that + 1.  It is never below hutk_ids_capacity (which alone is NOT a bound for a context with
 * a prefix: every match can add one more prefix).
 *
 * hutk_encode_special_batch_device: the arguments of hutk_encode_batch_device, work enqueued on hip_stream (NULL: the
 * context's stream).  Unlike that call it SYNCHRONISES THE STREAM ONCE, after the scan for matches: the host needs their
 * number to size the piece-wise encode.  With zero matches it then runs the plain encode straight into the caller's
 * buffers; otherwise cut, encode and stitch are enqueued and the call returns without waiting for them.  A context with a
 * regex pattern: HUTK_E_UNSUPPORTED at the call (as the token spans); ids_cap below hutk_special_ids_capacity() - 1:
 * HUTK_E_CAPACITY, nothing is enqueued; a NULL buffer: HUTK_E_ARG.  Alignment of d_ids_out: that of the element type;
 * 16 bytes gets the wide path (d_bytes: 16 bytes, else HUTK_E_ARG at the call, as the plain encode).  The special pieces are encoded too and their ids
 * dropped, so a marker that is not valid UTF-8 fails a character-mode context like any such text.  Runs on the context's
 * first device, serialised with the other calls on the context; the workspace grows by about 2 bytes per input byte
 * and, with matches, by a second id buffer.  hutk_encode_special_batch: host buffers (copies, calls the device form,
 * waits; one device, no chunking); returns HUTK_OK, the note HUTK_E_WORD_TOO_LARGE, or the error.
 * hutk_special_last_matches: the matches the last of these calls found.  hutk_debug_special_tile_bytes: the bytes one
 * workgroup of the scan owns (a match belongs to the workgroup that owns its first byte). */
int hutk_ctx_set_special_tokens(hutk_ctx* ctx, const uint8_t* bytes, const int64_t* offsets, const int32_t* ids, int64_t n);
int64_t hutk_ctx_special_token_count(const hutk_ctx* ctx);
int64_t hutk_special_ids_capacity(const hutk_ctx* ctx, int64_t n_bytes, int64_t n_docs);
int hutk_encode_special_batch_device(hutk_ctx* ctx, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                                     int64_t n_bytes, int32_t* d_ids_out, int64_t ids_cap, int64_t* d_out_offsets,
                                     int32_t* d_status, int32_t* d_err, void* hip_stream);
int hutk_encode_special_batch(hutk_ctx* ctx, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs,
                              int32_t* ids_out, int64_t ids_cap, int64_t* out_offsets, int32_t* status);
int64_t hutk_special_last_matches(const hutk_ctx* ctx);
int hutk_debug_special_tile_bytes(void);

/* DECODING with the set: ids -> text, the other direction of the calls above.  hutk_decode_batch and
 * hutk_decode_batch_device never look at the set (as the plain encode does not): they stay bit-exact with the reference
 * and refuse an id that is not a vocabulary line.
 *
 * An id is SPECIAL when some installed pair has it -- whether or not it is a vocabulary line as well, and even when that
 * line cannot be decoded.  Its STRING is the byte string of the first installed pair that carries the id (lowest index);
 * the bytes are written exactly as installed: a character-mode context maps no special-character values in them.
 *
 * flags == 0.  The special ids cut a document's ids into runs of ordinary ids.  The output is, in order, every run
 * decoded exactly as hutk_decode_batch decodes it AS A DOCUMENT OF ITS OWN, and every special's string.  So a context
 * with a prefix strips one prefix from the front of the first run and from the front of the run behind every special:
 * what hutk_encode_special_batch gave every text piece comes off again, and decode(encode(text)) is the text.
 * flags == HUTK_DECODE_SKIP_SPECIAL.  The output is exactly what hutk_decode_batch gives for the document with its special
 * ids deleted: they contribute nothing and cause no stripping (for a prefix vocabulary the prefix that stays is the
 * separator between the pieces).
 * An id that is neither special nor in [0, number of vocabulary lines): HUTK_DOC_ID_OUT_OF_RANGE and HUTK_E_VALUE -- also
 * an id just above the vocabulary, which never decodes as somebody's marker.  An ordinary id that cannot be decoded on
 * its own: HUTK_DOC_ID_UNDECODABLE and HUTK_E_UNSUPPORTED.  As in the plain decode such an id contributes no bytes, its
 * document is marked, every other token and document is exact.
 * No set installed: bytes, offsets, status and the error word are those of hutk_decode_batch_device, bit for bit.
 *
 * hutk_decode_special_batch_device: the arguments of hutk_decode_batch_device and `flags`, with its promises: bytes_out
 * == NULL gives out_offsets (the sizes) and status only, HUTK_E_CAPACITY in *d_err when the text does not fit bytes_cap
 * (nothing is written at or beyond it, offsets and status are complete), d_bytes_out may start at any byte address,
 * d_ids needs 4-byte alignment (16 take the faster loads).  The call is asynchronous on hip_stream (NULL: the context's)
 * and NEVER synchronises -- unlike the special encode it needs no count.  It runs on the context's first device,
 * serialised with the other calls on the context; the workspace grows by 4 bytes per id (a renumbered copy of the ids).
 * Refused at the call: flag bits other than HUTK_DECODE_SKIP_SPECIAL, a NULL context or buffer (HUTK_E_ARG), a host-only
 * context (HUTK_E_DEVICE).  Replacing or removing the set takes effect with the next call.
 * hutk_decode_special_batch: host buffers, staged like hutk_decode_batch and with its return codes. */
#define HUTK_DECODE_SKIP_SPECIAL 1
int hutk_decode_special_batch_device(hutk_ctx* ctx, const int32_t* d_ids, const int64_t* d_id_offsets, int64_t n_docs,
                                     int64_t n_ids, int flags, uint8_t* d_bytes_out, int64_t bytes_cap,
                                     int64_t* d_out_offsets, int32_t* d_status, int32_t* d_err, void* hip_stream);
int hutk_decode_special_batch(hutk_ctx* ctx, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs, int flags,
                              uint8_t* bytes_out, int64_t bytes_cap, int64_t* out_offsets, int32_t* status);

/* ---- byte fallback -----------------------------------------------------------------------------------------
 * SentencePiece-shaped vocabularies carry 256 lines "<0x00>".."<0xFF>": an item the vocabulary does not hold is
 * encoded as the ids of its bytes, and such an id decodes to its ONE raw byte.  The reference does neither: its encode
 * gives -1 for the item (core.c:205-207), its decode writes the six characters of the line.  hutk_encode_batch*,
 * hutk_decode_batch*, the special pair and the spans never look at the table: they stay bit-exact.
 *
 * THE TABLE.  int32[256]: the id of every byte value.
 *   hutk_ctx_find_byte_tokens  out256[b] = the id of the vocabulary key spelled exactly "<0xHH>" (two upper-case hex
 *       digits of b), -1 when there is none; returns how many were found.  The ids are those of the KEYS the loader read
 *       (the decode tables map the line "<0x0A>" to what the pretokenizer makes of it).  Works on a host-only context.
 *   hutk_ctx_set_byte_fallback installs ids256 in place of any earlier table, NULL removes it.  HUTK_E_VALUE, and the
 *       table in force stays, for an id < 0 or two equal ids.  Ids need not be vocabulary lines.  On a host-only context
 *       the table is validated and kept, no more.  A new context starts without one.
 *   hutk_ctx_byte_fallback     returns 1 and the table (out256 may be NULL) when one is installed, else 0.
 *
 * ENCODING.  The fallback encode of a document is its plain encode with every -1 replaced, in place and in order, by the
 * ids table[b] of the bytes b of the ONE item that the -1 covers (an item: see the token spans -- a byte with
 * is_byte_encoder, otherwise a character of 1..4 bytes, cut short at the document's end).  A -1 is never the product of
 * a merge and its neighbours never merge across it, so this is what a trainer-consistent SentencePiece encode gives.
 * Known ids, the order, status, a document cut at an over-long word and the note HUTK_E_WORD_TOO_LARGE are unchanged;
 * d_out_offsets describe the longer rows.
 * CAPACITY.  ids_cap >= hutk_ids_capacity() - 1 stays sufficient (with HUTK_FB_SPECIAL: hutk_special_ids_capacity() - 1).
 * Proof.  hutk_ids_capacity(b, d) = b U + d P + 1 allows U >= 1 ids for every input BYTE (U: the most units an item can
 * become) and P for a document's prefix.  An unknown item of l bytes was one unit -- one -1 -- of the plain encode and
 * becomes l ids; the bound already allows l U >= l ids for its l bytes, and no other id is added or changed.  With
 * HUTK_FB_SPECIAL the same holds for every text piece, and the proof of hutk_special_ids_capacity bounds the pieces.
 * PIPELINE.  The plain encode into a workspace; the byte spans of its ids (the kernels of hutk_token_spans_device, over
 * the workspace's CAPACITY, because the host never learns the number of ids: the ids behind the last document are a
 * document of no bytes whose spans nobody reads); then the expansion: counts per tile of 2048 ids, their scan, the write.
 * No workgroup of the expansion waits for another one.  The workspace grows by 12 bytes per id the capacity allows.
 * hutk_encode_fallback_batch_device: the arguments of hutk_encode_batch_device and flags: 0 or HUTK_FB_SPECIAL, which
 * cuts at the special tokens of hutk_ctx_set_special_tokens exactly as hutk_encode_special_batch_device does and encodes
 * the text pieces with fallback.  Asynchronous on hip_stream (NULL: the context's stream).  Without HUTK_FB_SPECIAL it
 * NEVER synchronises (once the workspace has grown); with it, once, where the special encode does.  Runs on the context's
 * first device, serialised with the other calls on the context.
 * Refused at the call: no table installed, a context with a regex pattern, a special-character replacement of several
 * units, a special-character entry for a byte >= 0x80 without is_byte_encoder, a token of 2 MiB or more
 * (HUTK_E_UNSUPPORTED: what the spans refuse); with HUTK_FB_SPECIAL an id that is both special and in the table
 * (HUTK_E_VALUE); unknown flag bits, a NULL buffer, more than 2^31 - 3 documents (HUTK_E_ARG); ids_cap below the bound
 * (HUTK_E_CAPACITY); a host-only context (HUTK_E_DEVICE).  Nothing is written at or beyond d_ids_out + ids_cap.
 * Alignment of d_ids_out: that of the element type; 16 bytes gets the wide path.  (d_bytes: 16 bytes, as for
 * hutk_encode_batch_device; anything else is HUTK_E_ARG at the call and nothing is written.)
 * A document whose spans do not verify (HUTK_DOC_SPAN_MISMATCH there: a special-character value that equals an ordinary
 * character, say) keeps its plain ids, -1 included, and its status; *d_err = HUTK_E_UNSUPPORTED; every other document is
 * exact.  Document offsets that do not describe the text, or a document of 2^31 bytes or more: *d_err = HUTK_E_ARG,
 * the outputs are undefined, nothing is read or written out of bounds.  n_docs == 0 and batches without ids write
 * offsets only and succeed.
 * hutk_encode_fallback_batch: host buffers (copies, calls the device form, waits; one device, no chunking); returns
 * HUTK_OK, the note HUTK_E_WORD_TOO_LARGE, or the error.
 *
 * DECODING.  The fallback decode is hutk_decode_batch_device (with HUTK_FB_SPECIAL: hutk_decode_special_batch_device,
 * HUTK_FB_SKIP_SPECIAL its HUTK_DECODE_SKIP_SPECIAL; the skip flag alone: HUTK_E_ARG) with one change: an id the table
 * carries decodes to its ONE raw byte, whatever its vocabulary line says -- also where no line has the id.  Such an id
 * is never stripped of a prefix, and it is no marker: the token behind it is not stripped, and the walk of
 * HUTK_FB_SKIP_SPECIAL from a document's first token to its first ordinary id ends on it.  So
 * decode_fallback(encode_fallback(text)) == text for every valid-UTF-8 text that decode(encode(text)) already gives
 * back apart from its -1s.  All promises of hutk_decode_batch_device carry over: d_bytes_out == NULL gives sizes only,
 * any output alignment, HUTK_E_CAPACITY with nothing written beyond bytes_cap, a bad id contributes nothing and marks
 * its document, the call never synchronises.  No table installed: HUTK_E_UNSUPPORTED; with HUTK_FB_SPECIAL an id that
 * is both special and in the table: HUTK_E_VALUE; a host-only context: HUTK_E_DEVICE.  The tables are those of the
 * special decode with 256 one-byte entries behind them; a pass over the ids renumbers table ids and special ids.
 * hutk_decode_fallback_batch: host buffers, staged like hutk_decode_batch and with its return codes. */
#define HUTK_FB_SPECIAL 1
#define HUTK_FB_SKIP_SPECIAL 2
int hutk_ctx_find_byte_tokens(const hutk_ctx* ctx, int32_t out256[256]);
int hutk_ctx_set_byte_fallback(hutk_ctx* ctx, const int32_t* ids256);
int hutk_ctx_byte_fallback(const hutk_ctx* ctx, int32_t* out256);
int hutk_encode_fallback_batch_device(hutk_ctx* ctx, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                                      int64_t n_bytes, int flags, int32_t* d_ids_out, int64_t ids_cap,
                                      int64_t* d_out_offsets, int32_t* d_status, int32_t* d_err, void* hip_stream);
int hutk_encode_fallback_batch(hutk_ctx* ctx, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, int flags,
                               int32_t* ids_out, int64_t ids_cap, int64_t* out_offsets, int32_t* status);
int hutk_decode_fallback_batch_device(hutk_ctx* ctx, const int32_t* d_ids, const int64_t* d_id_offsets, int64_t n_docs,
                                      int64_t n_ids, int flags, uint8_t* d_bytes_out, int64_t bytes_cap,
                                      int64_t* d_out_offsets, int32_t* d_status, int32_t* d_err, void* hip_stream);
int hutk_decode_fallback_batch(hutk_ctx* ctx, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs, int flags,
                               uint8_t* bytes_out, int64_t bytes_cap, int64_t* out_offsets, int32_t* status);

/* ---- Unicode normalisation --------------------------------------------------------------------------------
 * NFC, NFD, NFKC, NFKD of a packed batch in front of the encoders (hutk_normalize.hip): the pair
 * (uint8 bytes, int64 offsets[n_docs + 1]) in, the same pair out, so every *_batch_device call takes the result as it
 * is.  The reference has no counterpart (it encodes the bytes it is given).  For form F the output document is
 *     d.decode("utf-8", "surrogateescape") -> unicodedata.normalize(F, .) -> .encode("utf-8", "surrogateescape")
 * with the Unicode data of the tables' builder: exact at any length; documents are independent (a mark at the start
 * of a document never combines with the document before); every byte that strict UTF-8 rejects (a lone continuation
 * byte, an overlong form, an encoded surrogate, a value above U+10FFFF, a sequence the document's end cuts short) is
 * copied unchanged and normalisation never reaches across it; U+0000 is a character like any other.  Spans and
 * offsets computed afterwards are over the normalised text: nothing maps them back to the original bytes.
 *
 * A normaliser owns the tables on one device and a workspace; it needs no hutk_ctx and no vocabulary.  The tables are
 * one blob for all four forms, built by hutoken_amd/normalize.py from Python's unicodedata and written to a file by
 * `python -m hutoken_amd.normalize --write FILE`.  Format (little-endian 32-bit words; offsets in bytes from the
 * blob's start, multiples of 4):
 *   header, 32 words: 0 magic 0x4D524E48 ("HNRM")  1 format version (1)  2 Unicode version major << 16 | minor << 8 | patch
 *     3 size of the blob  4, 5 stage one: offset, entries (uint16[0x110000 >> 7]: block of code point c = stage1[c >> 7])
 *     6, 7 property blocks: offset, blocks (128 code points a block, two words a code point:
 *          word 0: bits 0..7 ccc | bit 8 + form: quick check "Yes" | bit 12: can be the second of a composite pair |
 *                  bits 16..23 / 24..31: ccc of the first character of the full canonical / compatibility decomposition;
 *          word 1: bits 0..15 / 16..31: word index of the canonical / compatibility decomposition, 0: none)
 *     8, 9 decompositions: offset, words (an entry: its length 1..18, then that many words code point | second << 21 |
 *          ccc << 24, fully expanded)   10, 11 composite pairs: offset, slots (a power of two of four-word slots
 *          {first, second, composite, 0}, first == 0xFFFFFFFF: empty; linear probing from the hash of the pair)
 *     12 pairs  13 block shift (7)  16..19 per form: the first lead byte that can start an unstable character
 *     20..23 per form: the largest output / input byte ratio of one character  24..27 per form: first unstable code point
 *   Hangul is composed and decomposed by arithmetic.  hutk_normalizer_create checks the magic, the version, every
 *   offset, index and length before anything reads through the blob: HUTK_E_VALUE with a message otherwise.
 * hutk_normalizer_info: out8 = format version, Unicode version word, blob bytes, chunk bytes, pairs, decomposition
 * words, the four lead bytes (one byte each, NFC lowest), the four ratios (likewise).
 *
 * hutk_normalize_batch_device: two calls, like the decode direction, asynchronous on hip_stream, neither synchronises.
 *   sizes call (d_out == NULL): d_out_offsets[n_docs + 1], d_changed[i] = the output of document i differs from its
 *     input (uint8[n_docs], may be NULL), d_totals[0] = output bytes, d_totals[1] = documents changed.
 *   write call (d_out, out_cap >= d_totals[0]): the text.  It uses the per-chunk state that the sizes call of the same
 *     batch (same form, pointers and sizes) left in the normaliser's workspace, so that call comes right before it;
 *     d_out_offsets, d_changed and d_totals may then be NULL and are left alone.  Without such a sizes call it runs
 *     the sizes stage itself first (d_out_offsets and d_totals are then required).
 * Work is cut into chunks of hutk_debug_norm_chunk_bytes() bytes of packed text; a chunk without a byte at or above the
 * form's first unstable lead byte is copied without a table access.  d_err (may be NULL) takes the first device-side
 * error: HUTK_E_ARG for offsets that do not rise from 0 to n_bytes (nothing else is then computed), HUTK_E_CAPACITY for an
 * out_cap below the total (nothing is written).  An unknown form, negative sizes, a missing buffer: HUTK_E_ARG at once;
 * no GPU: HUTK_E_DEVICE.  Calls on one normaliser are serialised (a mutex on the host, an event on the device).
 * Alignment of d_bytes and d_out: that of the element type (any byte address); 16 bytes gets the wide path.
 * hutk_normalize_batch: host arrays in; the work is done on the GPU; *out (offsets[n_docs] bytes of output at
 * (*out_offsets)[n_docs]) and *out_offsets (n_docs + 1 entries) are allocated here and given back with hutk_host_free. */
#define HUTK_NFC 0
#define HUTK_NFD 1
#define HUTK_NFKC 2
#define HUTK_NFKD 3
typedef struct hutk_normalizer hutk_normalizer;
int hutk_normalizer_create(hutk_normalizer** out, int device, const uint8_t* blob, int64_t n_blob_bytes);
void hutk_normalizer_destroy(hutk_normalizer* h);
int hutk_normalizer_info(const hutk_normalizer* h, int64_t* out8);
int hutk_normalize_batch_device(hutk_normalizer* h, int form, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                                int64_t n_bytes, uint8_t* d_out, int64_t out_cap, int64_t* d_out_offsets, uint8_t* d_changed,
                                int64_t* d_totals, int32_t* d_err, void* hip_stream);
int hutk_normalize_batch(hutk_normalizer* h, int form, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, uint8_t** out,
                         int64_t** out_offsets);
int hutk_debug_norm_chunk_bytes(void);

/* ---- Split presets: the GPT-2, cl100k (Llama 3) and Qwen2 pre-tokenisation ------------------------------------
 * The word split of byte-level BPE vocabularies on the device (hutk_presplit.hip).  A word starts
 * where regex.findall(pattern, d.decode("utf-8", "surrogateescape")) starts a match:
 *   HUTK_PRESPLIT_GPT2    's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+
 *   HUTK_PRESPLIT_CL100K  (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+
 *   HUTK_PRESPLIT_QWEN2   the same with \p{N} in place of \p{N}{1,3}
 * \p{L}, \p{N}: general categories L*, N* of the tables' Unicode version; \s: the 25 White_Space code points; under (?i:)
 * s also matches U+017F and no other letter has a partner outside ASCII.  A byte that strict UTF-8 rejects is one
 * character that is neither letter, number nor whitespace.  Documents are independent; every byte lies in some word.
 *
 * A pre-tokeniser owns the class tables on one device and a small workspace; it needs no hutk_ctx.  The tables are one
 * blob, built by hutoken_amd/pretokenize.py from Python's unicodedata and written to a file by
 * `python -m hutoken_amd.pretokenize --write FILE`.  Format (little-endian 32-bit words; offsets in bytes, multiples of 4):
 *   header, 16 words: 0 magic "HPTK" (0x4B545048), 1 version (1), 2 Unicode version (major << 16 | minor << 8 | patch),
 *     3 blob bytes, 4/5 stage one: offset, entries (uint16[0x110000 >> 7], the block of code point c), 6/7 class blocks:
 *     offset, blocks (8 words a block: two bits a code point, c at bits 2 * (c & 15) of word (c & 127) >> 4; 0 other,
 *     1 letter, 2 number, 3 whitespace), 8 the block shift (7).
 *   hutk_pretokenizer_create checks the magic, the version and every offset, size and block index before anything reads
 *   through them (HUTK_E_VALUE).
 *
 * hutk_pretokenize_batch_device: asynchronous on hip_stream, never synchronises (growing the workspace for a larger
 * batch than any before waits for the device once).  d_bytes at any alignment.  d_word_bits: n_bytes / 32 + 40 words;
 * bit p is set where a word starts, the bit at n_bytes is set, the rest is zero -- the bitmap the encoders take.  The
 * offsets are checked on the device: they rise from 0 to n_bytes, else HUTK_E_ARG in *d_err (may be NULL) and nothing
 * else is written.  Calls on one pre-tokeniser are serialised (a mutex on the host, an event on the device).
 *
 * hutk_pretokenize_starts_device turns the bitmap into positions, in two calls on the same stream: d_starts == NULL
 * counts (d_before: n_bytes / 32 + 2 values; afterwards d_before[n_bytes / 32 + 1] - 1 is the number of words); with
 * d_starts (room for that many) it writes the ascending byte positions of the word starts and d_start_offsets[n_docs + 1],
 * the index of every document's first word.  Behind a split that refused its offsets neither call reads the bitmap; on a
 * pre-tokeniser that has split nothing yet the bitmap is the caller's own and is counted as it is. */
#define HUTK_PRESPLIT_NONE (-1)
#define HUTK_PRESPLIT_GPT2 0
#define HUTK_PRESPLIT_CL100K 1
#define HUTK_PRESPLIT_QWEN2 2
typedef struct hutk_pretokenizer hutk_pretokenizer;
int hutk_pretokenizer_create(hutk_pretokenizer** out, int device, const uint8_t* blob, int64_t n_blob_bytes);
void hutk_pretokenizer_destroy(hutk_pretokenizer* h);
int hutk_pretokenize_batch_device(hutk_pretokenizer* h, int preset, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                                  int64_t n_bytes, uint32_t* d_word_bits, int32_t* d_err, void* hip_stream);
int hutk_pretokenize_starts_device(hutk_pretokenizer* h, const uint32_t* d_word_bits, const int64_t* d_offsets, int64_t n_docs,
                                   int64_t n_bytes, int64_t* d_before, int64_t* d_starts, int64_t* d_start_offsets, void* hip_stream);
/* On a context: hutk_ctx_set_pretokenizer installs a preset (HUTK_PRESPLIT_NONE removes it; tables / n_bytes: the blob,
 * uploaded once per device of the context, hutk_ctx_add_device's later ones included); hutk_ctx_pretokenizer reads it.
 * Every encode of the context -- hutk_encode_batch_device, hutk_encode_batch and its chunked path, hutk_encode, the
 * special-token and span calls -- then splits by the preset, on the device, with no copy down and no synchronisation; a
 * word of more than 262144 bytes ends its document in front of it (HUTK_DOC_WORD_TOO_LARGE), as with the built-in split.
 * HUTK_E_UNSUPPORTED: a context with a prefix (the presets are for byte-level vocabularies); a preset while a regex
 * pattern is set, and hutk_ctx_set_pattern while a preset is; the byte-fallback calls on a context with a preset. */
int hutk_ctx_set_pretokenizer(hutk_ctx* ctx, int preset, const uint8_t* tables, int64_t n_bytes);
int hutk_ctx_pretokenizer(const hutk_ctx* ctx);
/* the chunk of text one workgroup splits (tests lay their cases out around it) */
int hutk_debug_presplit_chunk_bytes(void);

/* ---- row-aligned features: row plans, the gather, word ids, answer positions ---------------------------------
 * ROW PLANS.  The geometry of the rows of a row layout as a device array, d_plan int64[n_rows][8] (8-byte aligned;
 * written with 16-byte stores when 16-byte aligned):
 *   d_plan[r] = {item, start, src_a, ka, col_a, src_b, kb, col_b}
 * item and start are what d_row_map holds: the document or pair of row r and the first id of its window inside the cut
 * side (padded rows and one-row pairs: item = r; start = 0, or under HUTK_COLLATE_TRUNC_LEFT the index of the first
 * kept id inside the document).  Column c of row r with col_a <= c < col_a + ka holds d_ids_a[src_a + (c - col_a)],
 * one with col_b <= c < col_b + kb holds d_ids_b[src_b + (c - col_b)]; every other column is bos, a separator, eos or
 * padding.  col_a and col_b include the shift of HUTK_COLLATE_PAD_LEFT.  Layouts without a B side write kb = 0,
 * src_b = 0 and col_b = col_a + ka.  Each planner takes the geometry arguments of its collate call and refuses what
 * that call refuses, runs one thread per row, and places a row with the device functions its collate kernel places it
 * with: the padded plan for the padded rows, the windows plan (d_row_offsets: from the windows rows call) for the
 * windows, the pair plan for both forms of the pairs (d_row_offsets == NULL: row i is pair i and n_rows == n_pairs).
 * *d_err receives HUTK_E_ARG for offsets outside their call's condition; the rows they describe are planned empty
 * (ka = 0, or kb = 0), and with offsets or row_offsets whose ends do not fit every row is.  Nothing is read outside the
 * offsets arrays.  n_docs == 0 / n_pairs == 0 writes nothing. */
int hutk_padded_plan_device(const int64_t* d_offsets, int64_t n_docs, int64_t n_ids, int64_t max_len, int32_t bos_id,
                            int32_t eos_id, int flags, int64_t* d_plan, int32_t* d_err, void* hip_stream);
int hutk_windows_plan_device(const int64_t* d_offsets, const int64_t* d_row_offsets, int64_t n_docs, int64_t n_ids,
                             int64_t n_rows, int64_t max_len, int64_t stride, int32_t bos_id, int32_t eos_id, int flags,
                             int64_t* d_plan, int32_t* d_err, void* hip_stream);
int hutk_pair_plan_device(const int64_t* d_offsets_a, const int64_t* d_offsets_b, const int64_t* d_row_offsets,
                          int64_t n_pairs, int64_t cap_a, int64_t cap_b, int64_t n_rows, int64_t max_len, int64_t stride,
                          int strategy, int32_t bos_id, const int32_t* sep_ids, int n_sep, int32_t eos_id, int flags,
                          int64_t* d_plan, int32_t* d_err, void* hip_stream);

/* THE GATHER.  Any per-token array in the rows' shape: d_out [n_rows][max_len] records of rec_bytes = 4, 8 or 16 (one
 * int32 or int64 per token, or a span of two), d_out[r][c] = d_values_a[src_a + (c - col_a)] on the A columns of plan
 * r, d_values_b[src_b + (c - col_b)] on its B columns, and *fill (one record on the HOST, copied into the launch) on
 * every other column.  d_values_a holds n_a records, d_values_b n_b; both may be one array.  Buffers are aligned to
 * their elements (4 bytes; 8 with rec_bytes 16); with max_len * rec_bytes a multiple of 16, d_out 16-byte aligned and
 * the values aligned to rec_bytes a thread stores 16 bytes at once.  The plan is not trusted: a side is clipped to the
 * columns [0, max_len), a negative ka or kb counts as 0, where both sides claim a column A holds it, and a record
 * outside its array is not read and leaves fill; each of these gives HUTK_E_ARG in *d_err.  Nothing is written outside
 * d_out.  n_rows == 0 writes nothing. */
int hutk_rows_gather_device(const int64_t* d_plan, int64_t n_rows, int64_t max_len, const void* d_values_a, int64_t n_a,
                            const void* d_values_b, int64_t n_b, int rec_bytes, const void* fill, void* d_out,
                            int32_t* d_err, void* hip_stream);

/* WORD IDS.  d_word_ids int32[n_ids]: the word of its document each token starts in, counted from 0, from the word
 * split of the packed text: d_word_bits as hutk_pretokenize_batch_device writes it, d_before the prefix counts of the
 * counting call of hutk_pretokenize_starts_device, d_offsets int64[n_docs + 1] the text offsets, d_spans [n_ids][2] the
 * BYTE spans of hutk_token_spans_device (span_width 4: int32, 8: int64), d_id_offsets int64[n_docs + 1].  With base the
 * text offset of the token's document, word_id = (set bits at positions base .. base + span_start) - 1.  One pass over
 * the ids, a search of the id offsets per tile of hutk_debug_word_ids_tile ids.  Verified, not trusted: a non-empty
 * span with a word start strictly inside it sets d_status[document] (int32[n_docs], may be NULL; cleared first) to
 * HUTK_DOC_SPAN_MISMATCH and *d_err to HUTK_E_UNSUPPORTED -- the ids were made under another split -- and the other
 * documents stay exact.  d_id_offsets[0] != 0, d_id_offsets[n_docs] != n_ids, d_offsets[0] < 0 or d_offsets[n_docs] >
 * n_bytes: HUTK_E_ARG in *d_err and nothing is written; a span outside its document's text: HUTK_E_ARG and -1. */
int hutk_token_word_ids_device(const uint32_t* d_word_bits, const int64_t* d_before, const int64_t* d_offsets,
                               int64_t n_docs, int64_t n_bytes, const void* d_spans, int span_width,
                               const int64_t* d_id_offsets, int64_t n_ids, int32_t* d_word_ids, int32_t* d_status,
                               int32_t* d_err, void* hip_stream);
int hutk_debug_word_ids_tile(void);

/* ANSWER POSITIONS.  d_out int32[n_rows][2]: the columns at which an answer starts and ends in every row, for
 * extractive QA.  side 0 names the A side of the plan, 1 the B side; d_spans [n_spans][2] are the spans of that side's
 * tokens (span_width 4 or 8), non-decreasing along a document; d_answers [n_items][2] of the same width holds (s, e) of
 * item i in the spans' unit, (-1, -1) or any s >= e for none.  The tokens of row r are j in [src, src + k) with spans
 * (a_j, b_j).  The answer lies in the row iff k > 0, a_src <= s and b_(src+k-1) >= e; then d_out[r] = {col + (max j:
 * a_j <= s) - src, col + (min j: b_j >= e) - src}, otherwise {-1, -1}.  One wavefront per row, two searches.  An item
 * outside [0, n_items), tokens outside [0, n_spans) or columns beyond int32: {-1, -1} and HUTK_E_ARG in *d_err. */
int hutk_rows_answers_device(const int64_t* d_plan, int64_t n_rows, int side, const void* d_spans, int span_width,
                             int64_t n_spans, const void* d_answers, int64_t n_items, int32_t* d_out, int32_t* d_err,
                             void* hip_stream);

/* MASKED-LM CORRUPTION.  d_input_ids [n_rows][max_len] elements of `width` bytes (4: int32, 8: int64) are rows whose
 * geometry d_plan holds; d_out_ids and d_labels are rectangles of the same shape and width.  A column is ELIGIBLE iff it
 * lies in the A side of its row's plan and sides has HUTK_MLM_SIDE_A, or in the B side and sides has HUTK_MLM_SIDE_B:
 * bos, separators, eos and padding never are.  Every draw is Philox4x32-10 (multipliers 0xD2511F53 and 0xCD9E8D57, key
 * increments 0x9E3779B9 and 0xBB67AE85) with key = (low32(seed), high32(seed)) and counter = (low32(row), high32(row),
 * unit, purpose), so it depends on nothing but (seed, row, unit, purpose): not on the batch a row sits in, the width
 * or the alignment.  purpose 0 with unit = column is the column's draw (u0, u1, u2, .); purpose 1 / 2 with unit = word
 * id is the draw of a word of side A / B (a B side counts its words from 0 again).
 *   token mode (d_words_a == NULL; n_a and n_b are not read): an eligible column is selected iff u0 < select_below.
 *   whole-word mode: d_words_a int32[n_a] and d_words_b int32[n_b] hold the word of every token of either side,
 *     indexed like the side's ids (hutk_token_word_ids_device); d_words_b == NULL reads both sides from d_words_a.  The
 *     word of column c of side X is d_words_x[src_x + (c - col_x)]; a word below 0 makes the column not eligible (the
 *     caller's way to protect a token, no error); otherwise the column is selected iff the word's u0 < select_below,
 *     and only a selected column makes its own draw for u1 and u2.
 *   a selected column: u1 < mask_below gives mask_id, else u1 < random_below gives the id (uint64(u2) * vocab_size) >>
 *     32, else the id stays; d_labels holds the original id.  Every other column: the id is copied and d_labels holds
 *     ignore_index.
 * The thresholds are integers in 0 .. 2^32 against draws of 32 bits (a probability p is int(p * 2^32)), with
 * 0 <= mask_below <= random_below <= 2^32; 1 <= vocab_size <= 2^31.  d_out_ids == d_input_ids is allowed (an element is
 * read and written by one thread); otherwise the three rectangles must not overlap.  Buffers are aligned to their
 * elements; with max_len a multiple of 4 and all three rectangles 16-byte aligned a thread moves four columns with
 * 16-byte loads and stores.  The plan is not trusted, as in the gather: a side is clipped to the columns [0, max_len), a
 * negative ka or kb counts as 0, where both sides claim a column it is A's, a word outside its array is not read; each
 * of these gives HUTK_E_ARG in *d_err (may be NULL) and the columns concerned are not eligible.  Nothing is written
 * outside the two outputs.  Refused with HUTK_E_ARG before a device is looked for: width other than 4 or 8, max_len
 * outside 1 .. 2^31 - 1, negative counts, thresholds outside their order or range, vocab_size outside 1 .. 2^31, sides
 * with unknown bits or none, an ignore_index that does not fit width, and with n_rows > 0 a NULL or misaligned buffer
 * or rectangles that overlap.  n_rows == 0 writes nothing.  Asynchronous on hip_stream; never synchronises. */
#define HUTK_MLM_SIDE_A 1
#define HUTK_MLM_SIDE_B 2
int hutk_rows_mlm_device(const int64_t* d_plan, int64_t n_rows, int64_t max_len, const void* d_input_ids, int width,
                         const int32_t* d_words_a, int64_t n_a, const int32_t* d_words_b, int64_t n_b,
                         uint64_t seed, int64_t select_below, int64_t mask_below, int64_t random_below,
                         int32_t mask_id, int64_t vocab_size, int64_t ignore_index, int sides,
                         void* d_out_ids, void* d_labels, int32_t* d_err, void* hip_stream);

/* LOSS LABELS.  d_labels [n_rows][max_len] of `width` bytes from the rows d_input_ids, their attention mask d_mask
 * uint8 [n_rows][max_len] and their plan.  real(c) = d_mask[r][c] != 0.  A real column is a LOSS column when it is in A
 * and flags has HUTK_LABELS_A; in B and HUTK_LABELS_B; a template column in front of col_b + kb and
 * HUTK_LABELS_TEMPLATE (bos and the separators); a template column at or behind col_b + kb and HUTK_LABELS_END (eos).
 * A layout without a B side writes col_b = col_a + ka and kb = 0, so the same rules hold for it.
 *   without HUTK_LABELS_SHIFT: d_labels[r][c] = loss(c) ? d_input_ids[r][c] : ignore_index;
 *   with it:                   d_labels[r][c] = real(c) && c + 1 < max_len && loss(c + 1) ? d_input_ids[r][c + 1]
 *                                                                                         : ignore_index
 * (what column c predicts: the last column of a row and the last pad column in front of a left-padded row predict
 * nothing).  With max_len a multiple of 4, d_input_ids and d_labels 16-byte aligned and d_mask 4-byte aligned a thread
 * moves four columns at once.  The plan is treated as in hutk_rows_mlm_device: clipped, A in front of B, HUTK_E_ARG in
 * *d_err for what does not fit the row, the columns concerned are template columns; col_b + kb is taken inside
 * [0, max_len].  Refused with HUTK_E_ARG before a device is looked for: width, max_len, n_rows and ignore_index as
 * there, flags with unknown bits or none of A, B, TEMPLATE and END, and with n_rows > 0 a NULL or misaligned buffer or
 * d_labels overlapping an input.  n_rows == 0 writes nothing.  Asynchronous on hip_stream; never synchronises. */
#define HUTK_LABELS_A 1
#define HUTK_LABELS_B 2
#define HUTK_LABELS_TEMPLATE 4
#define HUTK_LABELS_END 8
#define HUTK_LABELS_SHIFT 16
int hutk_rows_labels_device(const int64_t* d_plan, int64_t n_rows, int64_t max_len, const void* d_input_ids, int width,
                            const uint8_t* d_mask, int flags, int64_t ignore_index, void* d_labels, int32_t* d_err,
                            void* hip_stream);

/* SPAN CORRUPTION (T5-style).  d_input_ids [n_rows][max_len] elements of `width` bytes with their attention mask d_mask
 * uint8 [n_rows][max_len] and their plan -> the corrupted rows d_out_ids / d_out_mask of the same shape, in which every
 * noise span is ONE sentinel, and the target rows d_labels [n_rows][max_target_len] of the same width, in which the
 * spans follow their sentinels.  A row's outcome depends on (seed, the row's number, its plan and its mask) alone: not on
 * the batch, the width, the alignment or the tiling.  All numbers are exact integers; thresholds lie in 0 .. 2^32 and are
 * compared with draws of 32 bits, as in hutk_rows_mlm_device, whose generator this is.
 *   ELIGIBLE.  Column c is eligible iff it lies in a side of the clipped plan that `sides` names (HUTK_MLM_SIDE_*; the
 *     clipping is that of hutk_rows_mlm_device: a negative length counts as 0, a column both sides claim is A's) and
 *     d_mask[r][c] != 0.  side_end(c) is the clipped end of the side that holds c.
 *   DRAW.  An eligible column draws with purpose 3 and unit = c: (u0, u1, ., .).  It starts a span iff u0 < start_below,
 *     of the length len = 1 + #{ j in 0 .. n_len - 2 : u1 >= len_below[j] }; len_below is a HOST array of n_len
 *     cumulative thresholds, 1 <= n_len <= 32, non-decreasing, the last one 2^32, copied into the launch.  Then
 *     reach(c) = min(c + len, side_end(c)); for every column that starts nothing reach(c) = 0.
 *   NOISE.  noise0(c) = eligible(c) && max{ reach(s) : s <= c } > c, a prefix maximum along the row: spans that overlap
 *     or touch merge.  A run is a maximal run of noise0 columns; its number k is the count of runs that begin in front of
 *     it in the row, across both sides.  noise(c) = noise0(c) && k(c) < n_sentinels: whole runs past the last sentinel
 *     stay text.  sentinel(k) = sentinel_first + k * sentinel_step, the step being -1 or +1.
 *   CORRUPTED ROW.  real(c) = d_mask[r][c] != 0; keep(c) = real(c) && (!noise(c) || c begins its run).  The kept columns
 *     are written in order from column 0 of d_out_ids[r], a run's first column as its sentinel, every other one as its
 *     id; bos, separators and eos are real and never noise.  Whatever side the input is padded on, the output is compact:
 *     pad_id fills the rest, d_out_mask is 1 on the written columns and 0 behind, d_in_lengths[r] is their count.
 *   TARGET ROW.  For each run in order sentinel(k) and then the run's ids; then target_eos_id unless it is
 *     HUTK_NO_TOKEN; ignore_index fills the rest.  An element at a position >= max_target_len is dropped;
 *     d_tgt_lengths[r] is the count before that, eos included (a caller sees truncation as d_tgt_lengths[r] >
 *     max_target_len), and min(count, 2^31 - 1): the count passes that only with max_len above 1.43e9.
 *   DECODER INPUT.  With decoder_start_id other than HUTK_NO_TOKEN, d_decoder_ids of the target's shape:
 *     [r][0] = decoder_start_id, [r][p + 1] = d_labels[r][p] for p + 1 < max_target_len, pad_id where that is
 *     ignore_index.  Without, d_decoder_ids is not looked at and may be NULL.
 * One wavefront per row walks it in chunks of 256 columns; with max_len a multiple of 4, d_input_ids 16-byte and d_mask
 * 4-byte aligned a lane loads four columns at once.  The plan is trusted as little as in hutk_rows_mlm_device: what does
 * not fit the row gives HUTK_E_ARG in *d_err (may be NULL) and the columns concerned are not eligible; nothing is read
 * outside the rows and nothing is written outside the outputs.  Refused with HUTK_E_ARG before a device is looked for:
 * width other than 4 or 8, max_len or max_target_len outside 1 .. 2^31 - 1, n_rows < 0, start_below outside 0 .. 2^32, a
 * table that is empty, longer than 32, decreasing or not ending at 2^32, a step other than -1 and +1, n_sentinels < 0, a
 * first or last sentinel, a pad_id or an ignore_index that does not fit width, sides with unknown bits or none, and with
 * n_rows > 0 a NULL or misaligned buffer or an output that overlaps an input or another output (there is no in-place
 * form).  n_rows == 0 writes nothing.  Asynchronous on hip_stream; never synchronises. */
int hutk_rows_span_corrupt_device(const int64_t* d_plan, int64_t n_rows, int64_t max_len, const void* d_input_ids, int width,
                                  const uint8_t* d_mask, uint64_t seed, int64_t start_below, const int64_t* len_below,
                                  int n_len, int64_t sentinel_first, int sentinel_step, int64_t n_sentinels,
                                  int32_t target_eos_id, int32_t decoder_start_id, int64_t pad_id, int64_t ignore_index,
                                  int sides, int64_t max_target_len, void* d_out_ids, uint8_t* d_out_mask, void* d_labels,
                                  void* d_decoder_ids, int32_t* d_in_lengths, int32_t* d_tgt_lengths, int32_t* d_err,
                                  void* hip_stream);

/* ---- WordPiece: BERT's normaliser, word split and greedy longest match ------------------------------------------
 * The encoder of BERT-family vocabularies (a vocab.txt with "##" continuation pieces) on the device
 * (hutk_wordpiece.hip, hutk_wordpiece.h): the pair (uint8 bytes, int64 offsets[n_docs + 1]) in,
 * the ragged (int32 ids, int64 out_offsets[n_docs + 1]) of hutk_encode_batch_device out, so every collation, packing
 * and target call takes the result as it is.  The reference has no counterpart; the contract is the `tokenizers`
 * package: models.WordPiece behind normalizers.BertNormalizer and pre_tokenizers.BertPreTokenizer.  A document is
 * normalised, split into words, and every word is matched; documents are independent.
 *
 * NORMALISER, character by character, in this order (flags HUTK_WP_*):
 *   1. HUTK_WP_CLEAN_TEXT drops U+0000, U+FFFD and every character of category Cc, Cf or Co except \t \n \r (a dropped
 *      character joins its neighbours: "a" U+200B "b" is the word "ab"; Cn is not dropped), then maps every White_Space
 *      character that remains (25 code points, U+00A0, U+2028 and U+2029 among them) to ' '.  U+000B, U+000C and U+0085
 *      are Cc: they are dropped, they do not become spaces.
 *   2. HUTK_WP_CJK makes a word of every code point of 4E00-9FFF, 3400-4DBF, 20000-2A6DF, 2A700-2B73F, 2B740-2B81F,
 *      2B920-2CEAF, F900-FAFF, 2F800-2FA1F.  The sixth range starts at 2B920 as in `tokenizers`, not at 2B820 as in
 *      Google's BERT.
 *   3. HUTK_WP_STRIP_ACCENTS applies NFD (the normaliser above, on the same stream) and drops every character of
 *      category Mn.  Hangul syllables therefore become jamo.
 *   4. HUTK_WP_LOWERCASE maps every character on its own (Python's "".join(c.lower() for c in s)): no final-sigma rule,
 *      and U+0130 without HUTK_WP_STRIP_ACCENTS becomes 'i' + U+0307, two characters.
 *   A byte that strict UTF-8 rejects is not covered by `tokenizers`, which takes str.  It is one character of class
 *   "word" that stays as it is, as in the normaliser above; a sequence that a document's end cuts short is such bytes.
 * SPLIT.  Whitespace separates words and is dropped.  A punctuation character (ASCII 33-47, 58-64, 91-96, 123-126, or
 *   category P*) is a word of its own, and under HUTK_WP_CJK so is every CJK character.  Everything else runs together.
 * MATCH.  A word of more than max_input_chars_per_word characters (of the normalised word, not bytes) is one unk id.
 *   Otherwise from start = 0 the longest end on a character boundary such that word[start:end] is in the vocabulary is
 *   taken -- from the second piece on prefix + word[start:end] is looked up -- its id is emitted and the match goes on
 *   at end.  If no end matches at some start the whole word is one unk id and the pieces found so far are discarded:
 *   with "a" in the vocabulary and "##a" not, "aaa" is unk.  The id of a line is its number; of two equal lines the later
 *   id wins.  An empty or all-blank document gives no ids.
 * The classes and the lower-case mapping come from the Unicode data of the tables' builder (Python's unicodedata);
 * `tokenizers` carries tables of other versions, so the two differ on recently assigned characters (463 code points
 * with Unicode 13.0 against tokenizers 0.22.2, none below U+07FD).
 *
 * TABLES.  One blob, built by hutoken_amd/wordpiece.py and written to a file by `python -m hutoken_amd.wordpiece
 * --write FILE`.  Format (little-endian 32-bit words; offsets in bytes from the blob's start, multiples of 4):
 *   header, 32 words: 0 magic 0x43505748 ("HWPC")  1 format version (1)  2 Unicode version major << 16 | minor << 8 | patch
 *     3 size of the blob  4, 5 stage one: offset, entries (uint16[0x110000 >> 7]: block of code point c = stage1[c >> 7])
 *     6, 7 class blocks: offset, blocks (128 code points a block, one word a code point: bits 0..2 the class under
 *          HUTK_WP_CLEAN_TEXT -- 0 word, 1 space, 2 punctuation, 3 CJK, 4 dropped, 5 nonspacing mark | bits 3..23 the
 *          lower-case mapping's first character less the code point, modulo 2^21 | bits 24..26 the class without HUTK_WP_CLEAN_TEXT | bits 27..31 the
 *          index of the mapping's second character, 0: none)
 *     8, 9 second characters: offset, entries (uint32, entry 0 unused)   10 block shift (7)
 *     16..19 the largest characters-out / bytes-in of one code point through the normaliser, rounded up, for the settings
 *          lowercase | strip_accents << 1       20..23 the largest bytes-out / bytes-in, times 16, rounded up, likewise
 *   hutk_wordpiece_create checks the magic, the version, every offset, index and code point before anything reads
 *   through the blob: HUTK_E_VALUE with a message otherwise.
 *
 * hutk_wordpiece_create: a handle on one device (device < 0: the current one); it needs no hutk_ctx.  tables: the blob
 *   above; norm_blob: the normaliser's blob, needed with HUTK_WP_STRIP_ACCENTS and ignored (may be NULL) without;
 *   the vocabulary as n_vocab lines, line i being vocab_bytes[vocab_offsets[i] .. vocab_offsets[i + 1]).  HUTK_E_VALUE:
 *   an empty line, an unk_token that is no line, a prefix of more than 16 bytes, a max_input_chars_per_word outside
 *   0 .. 2^20, no line or 2^30 and more.  A line of more than 4 * max_input_chars_per_word bytes can never match and is
 *   kept for its id alone.  The table is built on the host and uploaded once: open addressing over (piece bytes, initial
 *   or continuation), 16 bytes a slot, a load of at most one half, continuation pieces stored without the prefix, all
 *   keys in one byte blob; a slot counts as a hit only after its bytes have been compared.
 * hutk_wordpiece_info: out8 = format version, Unicode version word, blob bytes, chunk bytes, vocabulary lines, table
 *   slots, flags, the unk id.
 * hutk_wordpiece_ids_capacity: an id covers at least one character of the normalised text, so n_bytes times header word
 *   16 + setting bounds the ids of any batch of n_bytes bytes (1 with the Unicode data seen so far: n_bytes itself).
 * hutk_wordpiece_encode_batch_device: asynchronous on hip_stream, never synchronises (growing the handle's workspace for
 *   a batch larger than any before may wait once).  d_ids[ids_cap], d_out_offsets[n_docs + 1]; d_word_ids (int32 per id,
 *   may be NULL): the index of the id's word in its document, what `tokenizers` calls word_ids.  d_err (may be NULL) takes
 *   the first device-side error: HUTK_E_ARG for offsets that do not rise from 0 to n_bytes (the kernels refuse before they
 *   read through them, and nothing else is written), HUTK_E_CAPACITY for an ids_cap below the total (no id is written).
 *   The text is cut into chunks of hutk_debug_wordpiece_chunk_bytes() bytes; a word may cross any number of chunk edges
 *   and have any length in bytes: its cost is bounded by max_input_chars_per_word characters walked and as many trips.
 *   Alignment of every buffer: that of its element type.  Calls on one handle are serialised.
 * hutk_wordpiece_encode_batch: host arrays in; the work is done on the GPU; *out_ids ((*out_offsets)[n_docs] entries),
 *   *out_offsets (n_docs + 1 entries) and, when out_word_ids is not NULL, *out_word_ids are allocated here and given
 *   back with hutk_host_free.
 * hutk_debug_wordpiece_bucket: the slot the probe of the piece starts at (tests build pieces that share one); -1 on bad
 *   arguments. */
#define HUTK_WP_CLEAN_TEXT 1u
#define HUTK_WP_CJK 2u
#define HUTK_WP_STRIP_ACCENTS 4u
#define HUTK_WP_LOWERCASE 8u
typedef struct hutk_wordpiece hutk_wordpiece;
int hutk_wordpiece_create(hutk_wordpiece** out, int device, const uint8_t* tables, int64_t n_table_bytes, const uint8_t* norm_blob,
                          int64_t n_norm_bytes, const uint8_t* vocab_bytes, const int64_t* vocab_offsets, int64_t n_vocab,
                          const char* unk_token, const char* prefix, int32_t max_input_chars_per_word, uint32_t flags);
void hutk_wordpiece_destroy(hutk_wordpiece* h);
int hutk_wordpiece_info(const hutk_wordpiece* h, int64_t* out8);
int64_t hutk_wordpiece_ids_capacity(const hutk_wordpiece* h, int64_t n_bytes, int64_t n_docs);
int hutk_wordpiece_encode_batch_device(hutk_wordpiece* h, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                                       int64_t n_bytes, int32_t* d_ids, int64_t ids_cap, int64_t* d_out_offsets,
                                       int32_t* d_word_ids, int32_t* d_err, void* hip_stream);
int hutk_wordpiece_encode_batch(hutk_wordpiece* h, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, int32_t** out_ids,
                                int64_t** out_offsets, int32_t** out_word_ids);
int hutk_debug_wordpiece_chunk_bytes(void);
int64_t hutk_debug_wordpiece_bucket(const hutk_wordpiece* h, const uint8_t* bytes, int64_t len, int continuation);

/* ---- Unigram: Metaspace word split and the best path over a word's piece lattice ---------------------------------
 * The encoder of SentencePiece-style Unigram vocabularies (T5, mT5, ALBERT, XLNet, XLM-R, mBART, Pegasus) on the device
 * (hutk_unigram.hip, hutk_unigram.h): the pair (uint8 bytes, int64 offsets[n_docs + 1]) in, the
 * ragged (int32 ids, int64 out_offsets[n_docs + 1]) of hutk_encode_batch_device out.  The reference has no counterpart;
 * the contract is the `tokenizers` package: models.Unigram(vocab, unk_id, byte_fallback=False) behind
 * pre_tokenizers.Metaspace(replacement U+2581, split=True), id for id and word id for word id.  Documents are independent.
 *
 * WORDS (flags HUTK_UG_*).  An empty document has no words.
 *   HUTK_UG_COLLAPSE_SPACES runs first: of a run of two or more U+0020 one stays (normalizers.Replace(" {2,}", " ")).
 *   Without HUTK_UG_WHITESPACE_SPLIT every U+0020 becomes U+2581 (a tab, a newline and U+00A0 are ordinary characters);
 *   with HUTK_UG_PREPEND (prepend_scheme "always") a U+2581 is put in front of the document unless it starts with a
 *   space or a literal U+2581; a word starts at every U+2581 and at the document's first character.  "a  b\tab" is
 *   U+2581 "a", U+2581, U+2581 "b\tab".  A literal U+2581 in the text acts exactly like a space.
 *   With HUTK_UG_WHITESPACE_SPLIT (pre_tokenizers.Sequence[WhitespaceSplit, Metaspace]; needs HUTK_UG_PREPEND) the words
 *   are the maximal runs of characters that are not White_Space (Rust's char::is_whitespace: U+0009-000D, 0020, 0085,
 *   00A0, 1680, 2000-200A, 2028, 2029, 202F, 205F, 3000); each run gets a U+2581 in front unless it starts with a
 *   literal one, and is split further at every literal U+2581 inside it.  The whitespace itself yields nothing.
 * PIECES of a word, taken as bytes b[0 .. n): encode_optimized with f64 scores.  unk_score = min(all scores) - 10,
 *   best[0] = 0.  For every character start s in rising order, m being the byte length of the character at s: every
 *   vocabulary piece equal to b[s .. s + L) is a candidate score(piece) + best[s] for position s + L, which replaces what
 *   the position holds if it holds nothing yet or if the candidate is strictly greater (so among equal scores the smallest
 *   s, the longest last piece, wins); if no piece equals the one character b[s .. s + m) the unknown piece (unk_id,
 *   unk_score) is a candidate for s + m by the same rule.  The path is walked back from n; consecutive ids equal to
 *   unk_id inside one word fuse into one (never across words; a line that sits at unk_id and matched literally counts).
 *   Of two equal lines the later id, with its own score, is the one found.  The additions are plain IEEE f64.
 *   A byte that strict UTF-8 rejects is a character of one byte that no piece matches (`tokenizers` takes str only: this
 *   is the library's own definition); a sequence that a document's end cuts short is such bytes.
 *
 * hutk_unigram_create: a handle on one device (device < 0: the current one); it needs no hutk_ctx.  Piece i of the
 *   n_pieces is piece_bytes[piece_offsets[i] .. piece_offsets[i + 1]) with scores[i]; its id is i.  HUTK_E_VALUE: no
 *   piece or 2^30 and more, an empty piece, a score that is not finite, an unk_id outside the vocabulary, a piece of
 *   more than 256 bytes (a U+2581 counted as one), HUTK_UG_WHITESPACE_SPLIT without HUTK_UG_PREPEND.  The table is built
 *   on the host and uploaded once: open addressing over the piece bytes, 16 bytes a slot, a load of at most one half,
 *   all keys in one byte blob, a slot a hit only after its bytes have been compared; the scores as f64 by id; per first
 *   byte a 64-bit mask of the key lengths that exist.  A key stores a leading U+2581 as the byte 0x20, as the folded
 *   text does.  A piece that holds a real space, a U+2581 anywhere but at its start, or ill-formed UTF-8 can never
 *   match and is kept for its id alone.
 * hutk_unigram_info: out8 = chunk bytes, pieces, table slots, flags, the unk id, the longest key in bytes, the length
 *   bound (256), the lanes of a group.
 * hutk_unigram_ids_capacity: n_bytes + n_docs.  An id covers at least one byte of the folded text, a byte of the source
 *   becomes at most one of the folded text, and the prefixes add at most one per document (a run's prefix under
 *   HUTK_UG_WHITESPACE_SPLIT takes the place of the whitespace in front of it); DESIGN.md section 8n has the proof.
 * hutk_unigram_encode_batch_device: asynchronous on hip_stream, never synchronises (growing the handle's workspace for
 *   a batch larger than any before may wait once).  d_ids[ids_cap], d_out_offsets[n_docs + 1]; d_word_ids (int32 per id,
 *   may be NULL): the index of the id's word in its document, what `tokenizers` calls word_ids.  d_err (may be NULL) takes
 *   the first device-side error: HUTK_E_ARG for offsets that do not rise from 0 to n_bytes (the kernels refuse before they
 *   read through them, and nothing else is written), HUTK_E_CAPACITY for an ids_cap below the total (no id is written).
 *   The text is cut into chunks of hutk_debug_unigram_chunk_bytes() bytes; a word may cross any number of chunk edges
 *   and has no length limit.  Alignment of every buffer: that of its element type.  Calls on one handle are serialised.
 * hutk_unigram_encode_batch: host arrays in; the work is done on the GPU; *out_ids ((*out_offsets)[n_docs] entries),
 *   *out_offsets (n_docs + 1 entries) and, when out_word_ids is not NULL, *out_word_ids are allocated here and given
 *   back with hutk_host_free.
 * hutk_debug_unigram_bucket: the slot the probe of the piece (its folded bytes) starts at (tests build pieces that share
 *   one); -1 on bad arguments. */
#define HUTK_UG_PREPEND 1u
#define HUTK_UG_WHITESPACE_SPLIT 2u
#define HUTK_UG_COLLAPSE_SPACES 4u
typedef struct hutk_unigram hutk_unigram;
int hutk_unigram_create(hutk_unigram** out, int device, const uint8_t* piece_bytes, const int64_t* piece_offsets, const double* scores,
                        int64_t n_pieces, int64_t unk_id, uint32_t flags);
void hutk_unigram_destroy(hutk_unigram* h);
int hutk_unigram_info(const hutk_unigram* h, int64_t* out8);
int64_t hutk_unigram_ids_capacity(const hutk_unigram* h, int64_t n_bytes, int64_t n_docs);
int hutk_unigram_encode_batch_device(hutk_unigram* h, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes,
                                     int32_t* d_ids, int64_t ids_cap, int64_t* d_out_offsets, int32_t* d_word_ids, int32_t* d_err,
                                     void* hip_stream);
int hutk_unigram_encode_batch(hutk_unigram* h, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, int32_t** out_ids,
                              int64_t** out_offsets, int32_t** out_word_ids);
int hutk_debug_unigram_chunk_bytes(void);
int64_t hutk_debug_unigram_bucket(const hutk_unigram* h, const uint8_t* bytes, int64_t len);

#ifdef __cplusplus
}
#endif
#endif /* HUTOKEN_AMD_H */
