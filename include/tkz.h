/*
 * tkz.h -- C ABI of libtkz, the MI355X-native batch BPE encoder.
 *
 * Drop-in boundary for ONE path of microsoft/Tokenizer's TokenizerLib: the plain Encode path
 *   TikTokenizer.Encode(string, List<int>, int, int)      Tokenizer_C#/TokenizerLib/TikTokenizer.cs:250-274
 *   BytePairEncoder.BytePairEncode(byte[], ranks)         Tokenizer_C#/TokenizerLib/Utils/BytePairEncoder.cs:13-76
 * reached through ITokenizer.Encode(text, allowedSpecial) / Encode(text, applySpecialTokens)
 * (Tokenizer_C#/TokenizerLib/ITokenizer.cs:12,28; TikTokenizer.cs:178-207).
 *
 * The reference has no FFI of its own; these entry points are what a
 * P/Invoke layer under `class GpuTikTokenizer : ITokenizer` binds (INTEGRATION.md shows the
 * DllImport stubs; bindings/csharp/ holds the class).  Plain pointers and sizes only; no exceptions
 * cross the boundary: every call returns a tkz_status and tkz_last_error() holds the message for
 * the calling thread.  There is NO CPU fallback: without a usable HIP device every encoder entry
 * point fails with TKZ_E_NO_DEVICE.
 *
 * Error mapping to the reference's exceptions:
 *   TKZ_E_FORMAT        InvalidOperationException(FormatException)   TikTokenizer.cs:114-136
 *   TKZ_E_DUP_RANK      ArgumentException                            TikTokenizer.cs:82-87
 *   TKZ_E_KEY_NOT_FOUND KeyNotFoundException                         BytePairEncoder.cs:17,73
 *   TKZ_E_UNSUPPORTED   NotImplementedException (unknown encoder)    TokenizerBuilder.cs:179
 */
#ifndef TKZ_H
#define TKZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum tkz_status {
    TKZ_OK = 0,
    TKZ_E_FORMAT = -1,
    TKZ_E_DUP_RANK = -2,
    TKZ_E_KEY_NOT_FOUND = -3,
    TKZ_E_CAPACITY = -4,      /* out_cap too small; *needed holds the required id count */
    TKZ_E_INVALID_UTF8 = -5,  /* the UTF-8 entry points require well-formed UTF-8 (a C# string always converts to it) */
    TKZ_E_ARG = -6,
    TKZ_E_UNSUPPORTED = -7,   /* pattern string that is not one of the three the reference defines; rank outside [0, 2^27) */
    TKZ_E_DEVICE = -8,        /* HIP runtime error */
    TKZ_E_NO_DEVICE = -9,     /* no HIP device / HIP runtime unusable: there is NO CPU fallback */
    TKZ_E_OUT_OF_MEMORY = -10 /* device memory for the workspace could not be allocated (OutOfMemoryException) */
} tkz_status;

/* The three split regexes the reference defines.  A pattern is an enum, not a regex string:
 * libtkz ships a hand-written scanner per pattern and refuses anything else.
 *   TKZ_PATTERN_P1            gpt2 / r50k_base / p50k_base / p50k_edit   TokenizerBuilder.cs:128,140,155,167
 *   TKZ_PATTERN_CL100K        cl100k_base                                TokenizerBuilder.cs:112
 *   TKZ_PATTERN_O200K_DOTNET  o200k_base as the C# reference runs it: the regex string of tokenizer_ts/src/tokenizerBuilder.ts:79-89 handed to
 *                             TokenizerBuilder.CreateTokenizer(stream, specials, pattern) (TokenizerBuilder.cs:210-213) and compiled by
 *                             `new Regex(pattern, RegexOptions.Compiled)` (TikTokenizer.cs:77): every class test looks at ONE UTF-16 code unit (a
 *                             supplementary-plane char is two "other" units whatever its Unicode class, and never the one-unit prefix of a
 *                             word), \s is .NET's (U+0085 is white space, U+FEFF is not) -- the semantics of the other two patterns.
 *   TKZ_PATTERN_O200K         the same string as the TypeScript reference runs it: `new RegExp(pattern, "gu")` (tokenizer_ts/src/tikTokenizer.ts:100),
 *                             one class test per code POINT, ECMAScript \s (U+FEFF is white space, U+0085 is not).
 * The two o200k variants agree on every text without supplementary-plane chars, U+0085 and U+FEFF. */
typedef enum tkz_pattern { TKZ_PATTERN_P1 = 1, TKZ_PATTERN_CL100K = 2, TKZ_PATTERN_O200K = 3, TKZ_PATTERN_O200K_DOTNET = 4 } tkz_pattern;
/* Which engine's reading of a regex string is wanted (tkz_pattern_from_regex_engine). */
typedef enum tkz_regex_engine { TKZ_ENGINE_DOTNET = 0, TKZ_ENGINE_ECMASCRIPT = 1 } tkz_regex_engine;

typedef struct tkz_vocab tkz_vocab;
typedef struct tkz_encoder tkz_encoder;

/* Message for the last failing call on this thread ("" if none). */
const char* tkz_last_error(void);

/* Replaces TikTokenizer.LoadTikTokenBpe(Stream) + Init's rank-collision check
 * (TikTokenizer.cs:99-139, :74-91).  `file` is the whole .tiktoken image (lines "base64 SP rank"). */
tkz_status tkz_vocab_from_tiktoken(const uint8_t* file, size_t n, tkz_vocab** out);
void tkz_vocab_destroy(tkz_vocab* v);
int64_t tkz_vocab_size(const tkz_vocab* v);
int32_t tkz_vocab_max_key_len(const tkz_vocab* v);
/* Entries of the (id_left, id_right) -> rank table built for the merge loop (informational). */
int64_t tkz_vocab_pair_table_entries(const tkz_vocab* v);
/* Bytes of one device table image (informational): 0 SHORT, 1 MID, 2 LONG (slots + blob), 3 PAIR,
 * 4 the direct-index tables (byte ids + byte-pair ranks); -1 = all of them.  0 for an unknown table. */
int64_t tkz_vocab_table_bytes(const tkz_vocab* v, int32_t which);
/* Encoder[key] on the host copy: rank of an exact byte string, or -1. */
int32_t tkz_vocab_rank(const tkz_vocab* v, const uint8_t* key, int32_t len);

/* The Unicode class the split scanners assign to code points first .. first + n - 1 (0 other, 1 Lu, 2 Ll, 3 Lt, 4 Lm, 5 Lo, 6 M, 7 N,
 * 8 white space: .NET's \s), from the table the device holds (Unicode 13.0, the data of the reference's net6.0 target).  Pattern 1 and
 * cl100k and TKZ_PATTERN_O200K_DOTNET look only code UNITS up (the entries below 0x10000); TKZ_PATTERN_O200K looks code points up
 * (and reads U+FEFF as white space, U+0085 as not).  Informational: lets a host verify the table. */
void tkz_unicode_classes(uint32_t first, int32_t n, uint8_t* out);

/* Map one of the reference's regex strings (exact text) to a tkz_pattern; anything else is
 * TKZ_E_UNSUPPORTED.  Replaces `new Regex(pattern, RegexOptions.Compiled)` (TikTokenizer.cs:77): the result has .NET's semantics
 * (the o200k string gives TKZ_PATTERN_O200K_DOTNET).  tkz_pattern_from_regex_engine names the engine: TKZ_ENGINE_ECMASCRIPT maps the
 * o200k string to TKZ_PATTERN_O200K (the TypeScript reference's reading) and refuses the other two strings, which libtkz implements
 * with .NET's semantics only. */
tkz_status tkz_pattern_from_regex(const char* regex_utf8, int32_t* pattern_out);
tkz_status tkz_pattern_from_regex_engine(const char* regex_utf8, int32_t engine, int32_t* pattern_out);

/* Replaces TokenizerBuilder.CreateTokenizer(stream, specials, pattern, cacheSize)
 * (TokenizerBuilder.cs:210-213) for the plain path: builds the device tables on HIP device
 * `device` (>= 0).  The vocab may be destroyed afterwards. */
tkz_status tkz_encoder_create(const tkz_vocab* v, int32_t pattern, int32_t device, tkz_encoder** out);
void tkz_encoder_destroy(tkz_encoder* e);
int32_t tkz_encoder_device(const tkz_encoder* e);
/* tkz_unicode_classes, read from the table image the encoder's DEVICE holds (downloaded for the call): verifies the upload. */
tkz_status tkz_encoder_unicode_classes(tkz_encoder* e, uint32_t first, int32_t n, uint8_t* out);

/* The HOST's Unicode classification.  The reference's split is whatever the running process's regex engine makes of \p{L}, \p{N}, \p{Lu} ... and \s
 * (`new Regex(pattern, RegexOptions.Compiled)`, TikTokenizer.cs:77): the categories of the runtime's Unicode data -- 13.0 under net6.0, 15.0 under .NET 8,
 * whatever the engine ships in Node.  libtkz is built with the 13.0 table (net6.0, the reference's target); a host on another runtime hands ITS table
 * over: classes[cp] in 0..8 (the codes of tkz_unicode_classes; 8 = what the host's \s matches) for cp < n_code_points, n_code_points = 65536 (a .NET host
 * classifies code UNITS: `char.GetUnicodeCategory` / `char.IsWhiteSpace` over the BMP is all pattern 1, cl100k and TKZ_PATTERN_O200K_DOTNET ever look
 * at) or 1114112 (every code point: TKZ_PATTERN_O200K).  The ASCII range keeps its classes (the same in every Unicode version) and a surrogate code
 * unit is class 0.  classes == NULL: the built-in table again.  Refused with TKZ_E_ARG while a call of the encoder is in flight. */
tkz_status tkz_encoder_set_unicode_classes(tkz_encoder* e, const uint8_t* classes, int64_t n_code_points);

/* Page-locked host memory for the buffers a host hands to the host-buffer entry points: copies from and to it run asynchronously at
 * the PCIe rate (tkz_encode_batch_utf8 cuts a batch of 12 MB or more into document ranges of 16 MB, keeps two launch sequences enqueued ahead and
 * overlaps the upload of a range with the kernels of the two before it and the download of the one before those -- results in memory from this
 * function leave on a copy engine of their own, tkz_encoder_engine_downloads; from pageable memory every copy is staged by the runtime first:
 * about half the rate).  A host without a HIP
 * binding of its own (C#, a plain C++ program) gets such memory here.  The memory is page-locked for every HIP device of the process
 * (hipHostMallocPortable), whichever device is current at the call.  tkz_host_free(NULL) is a no-op. */
tkz_status tkz_host_alloc(size_t bytes, void** out);
void tkz_host_free(void* p);

/* ---- the hot path ------------------------------------------------------------------------ */

/* EncodeBatch over HOST buffers: n_docs documents, document d = bytes[doc_offsets[d] .. doc_offsets[d+1]).
 * Each document is encoded exactly as ITokenizer.Encode(text, applySpecialTokens:false) would encode
 * the string it is the UTF-8 form of (with special tokens: tkz_encode_batch_special_utf8 / _device).  out_ids receives all ids, document after document;
 * out_offsets (n_docs+1 entries) the id range of each document.  Caller-allocated; out_cap >= total
 * bytes is always sufficient (a token is at least one byte).  On TKZ_E_CAPACITY nothing useful is
 * in out_ids and *needed (if non-NULL) holds the required capacity. */
tkz_status tkz_encode_batch_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets,
                                 int64_t n_docs, int32_t* out_ids, int64_t out_cap,
                                 int64_t* out_offsets, int64_t* needed);

/* Same with every buffer already resident in HBM on the encoder's device (d_bytes 16-byte aligned).
 * Work is enqueued on `hip_stream` (a hipStream_t, NULL = default stream); the call returns after
 * the stream has drained and *total_tokens is final (it is also the required capacity when the call
 * returns TKZ_E_CAPACITY).  For this and every other device entry: nothing outside d_bytes[0, total_bytes) is read
 * as text and no padding behind it is needed, nothing is written at or behind out_cap -- a successful call
 * leaves [*total_tokens, out_cap) as it found it -- or outside the n_docs + 1 entries of an offset array
 * (tests/test_gpu_buffer_contract.py). */
tkz_status tkz_encode_batch_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets,
                                   int64_t n_docs, int64_t total_bytes, int32_t* d_out_ids,
                                   int64_t out_cap, int64_t* d_out_offsets, void* hip_stream,
                                   int64_t* total_tokens);

/* EncodeBatch with special tokens: every document is encoded exactly as ITokenizer.Encode(text, allowedSpecial) would encode it (TikTokenizer.cs:178-207,
 * EncodeInternal / FindNextSpecialToken :141-170,230-241) -- the allowed literals are cut out of the text ON THE DEVICE, each becomes its id, and every plain
 * stretch between them is split as a text of its own.  allowed[k]: index into the literals registered by tkz_encoder_set_special_tokens (registration order =
 * the reference's alternation order: at one position the first registered literal that matches is the match, allowed or not; a literal never matches across a
 * document boundary).  n_allowed == 0, or no literal registered: the plain entry, launched exactly as it is.  An index out of range or given twice: TKZ_E_ARG.
 * The device path holds at most 256 registered literals of 1..128 bytes of well-formed UTF-8 with ids in [0, 2^26); with any other set registered these two
 * entries return TKZ_E_UNSUPPORTED (the callers' host segmentation is the fallback).  Buffers, capacity (out_cap >= total bytes is always sufficient), errors and
 * options as tkz_encode_batch_device / tkz_encode_batch_utf8; the host entry always takes the batch path (chunks are document ranges: no literal is cut).
 * Under o200k and under TKZ_OPT_PRETOK_SEQUENTIAL the launch sequence waits once for the number of segments.  Register special tokens while no call is in flight. */
tkz_status tkz_encode_batch_special_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                           const int32_t* allowed, int32_t n_allowed, int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets,
                                           void* hip_stream, int64_t* total_tokens);
tkz_status tkz_encode_batch_special_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed,
                                         int32_t n_allowed, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* needed);
/* informational: calls that took the device special path, special-token literals they turned into ids */
void tkz_encoder_special_stats(const tkz_encoder* e, int64_t* batches, int64_t* literals);

/* The same in two halves, for callers that keep several batches in flight (or do their own work while one runs):
 * _begin enqueues the batch on `hip_stream` and returns without waiting; _end waits for it, reports errors and
 * *total_tokens exactly as tkz_encode_batch_device, and frees the handle whatever it returns.  A batch that turns
 * out to need a larger internal buffer than its first attempt had (more pieces, longer miss lists, scratch for
 * pieces over 1024 bytes) is run again inside _end.  The buffers must stay valid, and the outputs unread, until
 * _end has returned.  Every pending call holds one workspace of the encoder: about 7 bytes per input byte on English / code text; text where
 * most pieces miss the vocabulary (CJK under an English table) makes the per-sub-tile miss lists grow from 64 entries towards 1024, i.e. from
 * 1.25 to at most 20 more bytes per input byte for that workspace -- they shrink again when later batches do not need them.
 * tkz_encoder_destroy while handles are outstanding is deferred: every such handle's _end returns TKZ_E_ARG and the last one frees the encoder. */
typedef struct tkz_pending tkz_pending;
tkz_status tkz_encode_batch_device_begin(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets,
                                         int64_t n_docs, int64_t total_bytes, int32_t* d_out_ids,
                                         int64_t out_cap, int64_t* d_out_offsets, void* hip_stream,
                                         tkz_pending** pending);
tkz_status tkz_encode_batch_device_end(tkz_pending* pending, int64_t* total_tokens);
/* _begin with a place for THIS batch's {n_docs, n_bytes, n_tokens}: d_counts3 (3 int64 on the device, the caller's, may be NULL) is written by
 * the batch's own stream work -- what tkz_comm_allgather_counts_device sends.  Final once _end has returned TKZ_OK (a batch that is run again
 * inside _end writes it again, on the same stream): enqueue the all-gather behind _end and any number of batches may be in flight, each with
 * its own block.  tkz_pending_counts_device returns d_counts3, or -- when it was NULL -- a block of the handle's workspace that is valid
 * until _end (for a gather enqueued between _begin and _end, which sees the FIRST attempt's counts: fine for a caller that treats a batch
 * whose _end reports anything but TKZ_OK, or that had to be run again, as failed). */
tkz_status tkz_encode_batch_device_begin_counts(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets,
                                                int64_t n_docs, int64_t total_bytes, int32_t* d_out_ids,
                                                int64_t out_cap, int64_t* d_out_offsets, void* hip_stream,
                                                int64_t* d_counts3, tkz_pending** pending);
const int64_t* tkz_pending_counts_device(const tkz_pending* pending);

/* EncodeBatch for hosts whose strings are UTF-16 (.NET `string`, Java, JavaScript): document d is the code units
 * units[unit_offsets[d] .. unit_offsets[d+1]).  The units are uploaded as they are and converted to UTF-8 ON THE
 * DEVICE exactly as Encoding.UTF8.GetBytes does (TikTokenizer.cs:261: a surrogate pair becomes one 4-byte char, a lone
 * surrogate -- also a pair cut by a document boundary -- becomes EF BF BD); the host is spared the transcode, which
 * is the slow half of feeding `string`s to the UTF-8 entry point.  Results as tkz_encode_batch_utf8;
 * out_cap >= 3 * total units is always sufficient.  Host buffers. */
tkz_status tkz_encode_batch_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets,
                                  int64_t n_docs, int32_t* out_ids, int64_t out_cap,
                                  int64_t* out_offsets, int64_t* needed);

/* The special and the trim entries for UTF-16 hosts: every document is encoded or trimmed exactly as ITokenizer.Encode(text, allowedSpecial) /
 * EncodeTrimSuffix(...) / EncodeTrimPrefix(...) treat the .NET `string` whose code units it is.  The transcode is the device's, as in tkz_encode_batch_utf16, and
 * the literal search reads what .NET reads: FindNextSpecialToken searches the UTF-16 string, where a lone surrogate -- a high half without its low half, a low
 * half without its high half, either half of a pair a document boundary cuts -- is NOT U+FFFD, although its bytes after the transcode are EF BF BD.  The
 * transcoder therefore marks every U+FFFD it wrote itself; a registered literal that holds U+FFFD does not match over such a byte and the alternation goes on to
 * the next registered literal (a U+FFFD that is in the string matches as ever).  With no such literal registered nothing is marked and nothing is read.
 *   tkz_encode_batch_special_utf16: allowed / n_allowed, TKZ_E_ARG, TKZ_E_UNSUPPORTED and tkz_encoder_special_stats as tkz_encode_batch_special_utf8; buffers,
 *     chunks (document ranges: no literal is cut), page-locked fast paths and results as tkz_encode_batch_utf16, which it IS when n_allowed == 0 or nothing is
 *     registered.  out_cap >= 3 * total units is always sufficient.
 *   tkz_encode_batch_trim_utf16: side, max_tokens, max_tokens_per_doc (a HOST array, a negative entry is TKZ_E_ARG), out_cap (the KEPT ids), TKZ_E_CAPACITY with
 *     *needed and every other error as tkz_encode_batch_trim_utf8.  cut_units[d] (n_docs entries, may be NULL): the reference's encodeLength /
 *     actualPrefixStrLength, i.e. the kept (suffix) or dropped (prefix) text is the first cut_units[d] code units of document d; a replaced surrogate counts as the
 *     one unit it is.  There is no cut_bytes: the bytes never exist on the host.  The WHOLE batch is staged and transcoded on the device, then ONE trim call.
 * Host buffers.  No code units (all offsets 0): zero offsets and zero cut_units. */
tkz_status tkz_encode_batch_special_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed,
                                          int32_t n_allowed, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* needed);
tkz_status tkz_encode_batch_trim_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                       int32_t side, int64_t max_tokens, const int64_t* max_tokens_per_doc, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                       int64_t* cut_units, int64_t* needed);

/* Single-string entries for `string` callers.  UTF-16: the split sees the code units as .NET's Regex
 * does (a supplementary-plane char is two "other" units, a lone surrogate one); each piece is
 * converted as Encoding.UTF8.GetBytes does (lone surrogate -> EF BF BD), TikTokenizer.cs:261. */
tkz_status tkz_encode_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, int32_t* out_ids,
                           int64_t out_cap, int64_t* n_out);
tkz_status tkz_encode_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, int32_t* out_ids,
                            int64_t out_cap, int64_t* n_out);

/* ITokenizer.Encode(text, allowedSpecial) on ONE string (TikTokenizer.cs:178-207; Encode(text, applySpecialTokens: true) is the call with every registered
 * literal allowed).  The ids are tkz_encode_batch_special_utf8's / _utf16's for the same text as a batch of one document; allowed / n_allowed, TKZ_E_ARG and
 * TKZ_E_UNSUPPORTED as there.  A text the plain single entries send through the single-launch kernel (at most 128 KiB of UTF-8; o200k: 1 KiB) goes through
 * ONE launch here as well -- literal search, split, lookups, merges and ids --; a longer text, and one the kernel hands back (a piece of more than 1 KiB, a
 * missed piece of more than 256 bytes, an error to report), takes the batch entry's path.  n_allowed == 0 or nothing registered: tkz_encode_utf8 /
 * tkz_encode_utf16, and tkz_encoder_special_stats does not move.  A successful call counts as one batch there, with the literals it turned into ids; a call
 * that takes the launch counts in tkz_encoder_small_path_calls.  TKZ_E_CAPACITY: *n_out is the required count.
 *   tkz_encode_special_utf16: the transcode is the host's, as in tkz_encode_utf16; with a registered literal that holds U+FFFD the same loop notes where a
 *   U+FFFD stands for a lone surrogate, which such a literal does not match (see tkz_encode_batch_special_utf16). */
tkz_status tkz_encode_special_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t* out_ids,
                                   int64_t out_cap, int64_t* n_out);
tkz_status tkz_encode_special_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t* out_ids,
                                    int64_t out_cap, int64_t* n_out);

/* EncodeBatch with PIECE granularity -- what EncodeTrimSuffix / EncodeTrimPrefix consume
 * (TikTokenizer.cs:288-341 and :483-519 walk the regex matches of a text and need the token count and
 * the length of each).  Every document is split into its pieces and each piece is encoded:
 * piece k = bytes[piece_byte_offsets[k] .. piece_byte_offsets[k+1]), its ids are
 * out_ids[piece_token_offsets[k] .. piece_token_offsets[k+1]); the pieces of document d are
 * [doc_piece_offsets[d], doc_piece_offsets[d+1]).  piece_cap is the capacity of the two piece arrays
 * minus one (piece_cap >= total bytes is always enough); TKZ_E_CAPACITY with *n_pieces / *needed_ids
 * holding the required sizes otherwise.  Host buffers.  One launch sequence: the piece offsets are built on the device from
 * the piece-start bitmap and the encode kernels mark the token position of every piece start. */
tkz_status tkz_encode_batch_pieces_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets,
                                        int64_t n_docs, int32_t* out_ids, int64_t out_cap,
                                        int64_t* doc_piece_offsets, int64_t* piece_byte_offsets,
                                        int64_t* piece_token_offsets, int64_t piece_cap,
                                        int64_t* n_pieces, int64_t* needed_ids);

/* EncodeTrimSuffix / EncodeTrimPrefix for a batch, ON THE DEVICE (TikTokenizer.cs:288-579): every document is cut to at most a maximum of tokens exactly as
 * EncodeTrimSuffix(text, allowedSpecial, maxTokenCount) / EncodeTrimPrefix(...) cut the string it is the UTF-8 form of.  The items of a document are the regex
 * pieces of its plain stretches and one item of one token per allowed literal, in order; a piece of several tokens is never split.
 *   TKZ_TRIM_SUFFIX keeps the longest run of leading items whose tokens sum to at most the maximum (the reference's loop with its two `break`s, :296-340,:356-378);
 *   TKZ_TRIM_PREFIX keeps everything when the document has at most the maximum, else drops the items up to the first item boundary whose cumulative token count
 *                   is at least count - maximum (TrimPrefix, :470-483).
 * d_out_ids / d_out_offsets (n_docs + 1): the KEPT ids, compacted, document after document.  d_cut_bytes[d]: bytes of the kept text (suffix) or of the dropped text
 * (prefix); d_cut_units[d]: the same length in UTF-16 code units -- the reference's encodeLength / actualPrefixStrLength: one per non-continuation byte and one more
 * per byte >= 0xF0 --; a document kept whole reports its full length for suffix and 0 for prefix.  Either array may be NULL (n_docs entries each, on the device).
 * The maximum: d_max_tokens == NULL: max_tokens for every document (negative: TKZ_E_ARG -- the reference's prefix variant returns the whole text then: a quirk the
 * callers keep on the host); else d_max_tokens[d] for document d (device; max_tokens is ignored), where a NEGATIVE ENTRY COUNTS AS 0.
 * allowed / n_allowed exactly as tkz_encode_batch_special_device (registration order, TKZ_E_ARG for a bad index, TKZ_E_UNSUPPORTED for a set beyond the device
 * path); n_allowed == 0: no literal is looked for and no literal kernel is launched.
 * out_cap counts the KEPT ids only -- min(total_bytes, n_docs * maximum) is always sufficient --: the untrimmed ids live in the workspace, never in the caller's
 * buffer.  On TKZ_E_CAPACITY nothing is in d_out_ids and *total_tokens / *needed hold the kept total; the encoder's {n_docs, n_bytes, n_tokens} block receives the
 * kept token count.  Errors (invalid UTF-8, TKZ_E_KEY_NOT_FOUND, pieces beyond 2^30 bytes, workspace growth) as tkz_encode_batch_device; a batch that has to be run
 * again is run again inside the call, which returns after the stream has drained (it also waits once, inside, for the number of pieces).
 * Workspace: the batch path's ~7 bytes per input byte, and 8 more per input byte (the untrimmed ids and a token mark per possible piece, 4 each), 16 per PIECE
 * (its byte and token offset: ~3.6 per input byte on English text, at most 16) and 32 per document.  The per-piece arrays never leave the device.
 * tkz_encode_batch_trim_utf8: the same over host buffers (max_tokens_per_doc is a HOST array, a negative entry is TKZ_E_ARG).  It stages the WHOLE batch on the
 * device, as tkz_encode_batch_pieces_utf8 does, and copies its result from ONE call of the device entry: no chunk pipeline, no single-launch path (ONE text: see
 * tkz_encode_trim_utf8 below, which has one). */
typedef enum tkz_trim_side { TKZ_TRIM_SUFFIX = 0, TKZ_TRIM_PREFIX = 1 } tkz_trim_side;
tkz_status tkz_encode_batch_trim_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                        const int32_t* allowed, int32_t n_allowed, int32_t side, int64_t max_tokens, const int64_t* d_max_tokens,
                                        int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets, int64_t* d_cut_bytes, int64_t* d_cut_units,
                                        void* hip_stream, int64_t* total_tokens);
tkz_status tkz_encode_batch_trim_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                      int32_t side, int64_t max_tokens, const int64_t* max_tokens_per_doc, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                      int64_t* cut_bytes, int64_t* cut_units, int64_t* needed);

/* EncodeTrimSuffix / EncodeTrimPrefix on ONE string (TikTokenizer.cs:288-579): "cut this prompt to max_tokens tokens and tell me what text is left".  The kept
 * ids, *cut_bytes and *cut_units are what tkz_encode_batch_trim_utf8 / _utf16 return for the same text as a batch of one document with the uniform maximum
 * max_tokens: the kept length for TKZ_TRIM_SUFFIX, the dropped length for TKZ_TRIM_PREFIX; a text kept whole reports its full length for suffix and 0 for
 * prefix.  side, allowed / n_allowed, TKZ_E_ARG (a bad side, a negative maximum, a bad or repeated index, a null n_out) and TKZ_E_UNSUPPORTED exactly as there.
 * cut_bytes and cut_units may each be NULL.  out_cap counts the KEPT ids only; on TKZ_E_CAPACITY *n_out is the kept count.  len == 0: TKZ_OK, *n_out == 0, zero
 * cuts.  n_allowed == 0 or nothing registered: a plain trim, no literal is looked for and tkz_encoder_special_stats does not move; a call with literals moves it
 * by what the batch trim entry moves it by for that text (a call that fails with TKZ_E_CAPACITY, there as here: the literals taken are counted, the batch is not).
 * Route: a text of at most 96 KiB of UTF-8 that the plain single entries send through the single-launch kernel (o200k: 1 KiB) is ONE launch here as well --
 * literal search, split, lookups, merges, ids, the cut and its lengths; the host copies the kept range of the ids out of the page-locked block -- and counts in
 * tkz_encoder_small_path_calls.  (96 KiB, not the plain entries' 128 KiB: beyond it the batch trim path, which costs the same at every size, is as fast or faster.)  Any other text, and one the kernel hands back (a piece of more than 1 KiB, a missed piece of more than 256 bytes, an error to
 * diagnose, lists to grow: the second figure of tkz_encoder_small_path_calls), takes the batch trim entry's path with identical results.
 *   tkz_encode_trim_utf16: the transcode is the host's, as in tkz_encode_special_utf16, the replaced-byte bitmap in the same loop when a registered literal holds
 *   U+FFFD; a replaced surrogate counts as the one unit it is.  A call that does not take the launch is tkz_encode_batch_trim_utf16's with the code units. */
tkz_status tkz_encode_trim_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t side, int64_t max_tokens,
                                int32_t* out_ids, int64_t out_cap, int64_t* n_out, int64_t* cut_bytes, int64_t* cut_units);
tkz_status tkz_encode_trim_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t side, int64_t max_tokens,
                                 int32_t* out_ids, int64_t out_cap, int64_t* n_out, int64_t* cut_units);

/* ---- Count: Encode(...).Count for a batch or one text, without the ids ------------------------------
 * What prompt budgeting, length filtering and bucketing ask of a tokenizer: how many tokens every document has.  out_offsets (n_docs + 1 entries) is EXACTLY what the
 * matching encode entry writes for the same arguments -- tkz_encode_batch_special_* when n_allowed > 0 and literals are registered, the plain entry otherwise --;
 * the count of document d is out_offsets[d + 1] - out_offsets[d], *total_tokens (may be NULL) the last entry.  No id buffer is taken, none is allocated and no id
 * is stored or copied: on the device k_tokcount stands where k_place stands in the launch sequence (everything before it -- marks, literals, pre-tokenizer, probe,
 * merges, scans, retries, learning -- and k_docoffs behind it are the encode call's, so a count call trains and promotes as an encode call does); a sub-tile in which no
 * document starts is skipped, one with document starts is read up to its last one.  The host entries stage no ids and download none: only the offsets travel back.
 * allowed / n_allowed, TKZ_E_ARG, TKZ_E_UNSUPPORTED and tkz_encoder_special_stats as tkz_encode_batch_special_device / _utf8 / _utf16.  Every other error as in the
 * encode entries (TKZ_E_INVALID_UTF8, TKZ_E_KEY_NOT_FOUND, bad offsets or null buffers: TKZ_E_ARG); TKZ_E_CAPACITY is never returned.  An empty batch or text:
 * TKZ_OK and offsets of zero -- the host entries launch nothing, the device entry clears d_out_offsets on the stream.  d_bytes 16-byte aligned, as for every device entry.
 *   tkz_count_batch_utf8 / _utf16: the routes of tkz_encode_batch_utf8 / _utf16 -- a small plain UTF-8 batch is ONE launch of the single-launch kernel as it is (its
 *     ids land in the encoder's page-locked block and stay there; tkz_encoder_small_path_calls moves as for the encode call), anything else the chunk pipeline.
 *   tkz_count_utf8 / _utf16: ONE text, *n_out its count (n_out may not be NULL).  The routes of tkz_encode_utf8 / tkz_encode_special_utf8 and their UTF-16 forms: the
 *     UTF-16 text is transcoded on the host, a text with literals takes the special form of the single launch under the same rule.
 * There is no _begin / _end form. */
tkz_status tkz_count_batch_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                  const int32_t* allowed, int32_t n_allowed, int64_t* d_out_offsets, void* hip_stream, int64_t* total_tokens);
tkz_status tkz_count_batch_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                int64_t* out_offsets, int64_t* total_tokens);
tkz_status tkz_count_batch_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                 int64_t* out_offsets, int64_t* total_tokens);
tkz_status tkz_count_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t* n_out);
tkz_status tkz_count_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t* n_out);
/* informational: successful count calls, and those of them the single-launch kernel answered */
void tkz_encoder_count_calls(const tkz_encoder* e, int64_t* calls, int64_t* single_launch);

/* ---- Token spans: which part of the text is token t (offset_mapping, decode_with_offsets, EncodeToTokens' Offset) ----
 * The ids and out_offsets (n_docs + 1 entries) are EXACTLY those of the matching encode entry for the same arguments -- tkz_encode_batch_special_* when n_allowed > 0
 * and literals are registered, the plain entry otherwise.  For document d with tokens out_offsets[d] .. out_offsets[d + 1], token t also gets
 *   tok_bytes[t] (int32)  the offset of the token's first byte from the start of ITS DOCUMENT, in the document's UTF-8 form.  The spans partition the document: its
 *                         first token has 0, token t ends where t + 1 starts, the last one ends at the document's length, and the bytes in between are the
 *                         vocabulary key of ids[t] (the literal, for an allowed special token);
 *   tok_units[t] (int32)  the same position in UTF-16 code units, by the rule of cut_units (tkz_encode_batch_trim_device): the number of units BEGUN in
 *                         [document start, token start) -- one per non-continuation byte and one more per byte >= 0xF0.  So
 *                           - a token that starts inside a multi-byte character (byte-level BPE does that to emoji and CJK under an English vocabulary) starts
 *                             AFTER that character's units: for F0 9F 98 80 split into several tokens the first token carries both units;
 *                           - a token made of continuation bytes only has an EMPTY unit span (it starts where the next token starts);
 *                           - (UTF-16 entries) a lone surrogate, which the transcoder replaced by EF BF BD, counts as the one unit it is.
 * Either array may be NULL, not both (TKZ_E_ARG); each has out_cap entries, as the ids have.  A document of 2^31 bytes or more is TKZ_E_UNSUPPORTED for these
 * entries only: the host entries see it in the offsets, the device entry learns it from the device, like its other device-side errors.
 *   tkz_encode_batch_spans_device: device buffers.  Errors, retries, workspace growth and TKZ_E_CAPACITY (*total_tokens the required count, nothing promised in
 *     the outputs) as tkz_encode_batch_trim_device; allowed / n_allowed and tkz_encoder_special_stats as tkz_encode_batch_special_device.  An empty batch clears
 *     d_out_offsets on the stream.  The launch sequence is the piece-granular one of the trim entry (it waits once, inside, for the number of pieces), the ids go
 *     straight into d_out_ids; behind it k_tokspan_mark, k_tokspan_count, two scans and k_tokspan_write.  Workspace beyond the trim entry's piece arrays: a bit per
 *     input byte and 24 bytes per KiB.  One lane walks the ids of a piece of several tokens: a single piece of many megabytes is walked by one lane.
 *   tkz_encode_batch_spans_utf8: host buffers.  The WHOLE batch is staged, ONE call of the device entry, the results downloaded, as tkz_encode_batch_trim_utf8:
 *     no chunk pipeline, no single-launch route.
 *   tkz_encode_batch_spans_utf16: code units in, transcoded on the device as tkz_encode_batch_trim_utf16; unit_offsets and tok_units in code units.  There is no
 *     tok_bytes: the bytes never exist on the host.  Literals that hold U+FFFD as in the other UTF-16 special entries.
 *   tkz_encode_spans_utf8 / _utf16: ONE text -- the batch entry with one document, at every size.  TKZ_E_ARG for a negative len or a null n_out; *n_out is the
 *     required count on TKZ_E_CAPACITY.
 * There is no _begin / _end form. */
tkz_status tkz_encode_batch_spans_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                         const int32_t* allowed, int32_t n_allowed, int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets,
                                         int32_t* d_tok_bytes, int32_t* d_tok_units, void* hip_stream, int64_t* total_tokens);
tkz_status tkz_encode_batch_spans_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                       int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int32_t* tok_bytes, int32_t* tok_units, int64_t* needed);
tkz_status tkz_encode_batch_spans_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                        int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int32_t* tok_units, int64_t* needed);
tkz_status tkz_encode_spans_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t* out_ids, int64_t out_cap,
                                 int32_t* tok_bytes, int32_t* tok_units, int64_t* n_out);
tkz_status tkz_encode_spans_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t* out_ids, int64_t out_cap,
                                  int32_t* tok_units, int64_t* n_out);
/* informational: successful calls of the span entries */
void tkz_encoder_spans_calls(const tkz_encoder* e, int64_t* calls);

/* ---- Token-budget chunks: a document cut into pieces of at most max_tokens tokens, in ONE call ----
 * What a caller gets by calling EncodeTrimSuffix(rest, allowedSpecial, max_tokens), taking the returned text off the front and calling again to the end of the
 * document -- without a call a chunk, without encoding the remainder again, and without the loop that never ends when the next piece alone exceeds the budget.
 * THE RULE.  The items of a document are those of the trim entries (TikTokenizer.cs:288-341): the regex pieces of its plain stretches and one item of one token per
 * allowed literal, in order.  Chunks partition the document's tokens:
 *   - a chunk starts at token s; the first chunk starts at the document's first token;
 *   - it ends at the largest item boundary b with s < b <= s + max_tokens;
 *   - if there is no such boundary, the item at s still has more than max_tokens tokens left, and the chunk ends at s + max_tokens, inside that item;
 *   - the next chunk starts where this one ended.
 * So: while no item exceeds the budget the chunks are exactly the results of the repeated EncodeTrimSuffix loop, ids and texts alike; an item over the budget is cut
 * into runs of max_tokens, and its last partial run begins a chunk that goes on taking the items that follow; no chunk is empty and none exceeds max_tokens; an
 * empty document has no chunks; max_tokens < 1 is TKZ_E_ARG.
 * POSITIONS follow the span entries' rules.  Bytes: the byte start of a chunk that begins inside an item is the item's byte start plus the key lengths of the item's
 * tokens in front of it.  UTF-16 units: the number of units BEGUN in [document start, chunk start) -- one per non-continuation byte and one more per byte >= 0xF0;
 * a cut inside a character therefore leaves the whole character, and a surrogate pair, to the earlier chunk.  (UTF-16 entries) a lone surrogate, which the
 * transcoder replaced by EF BF BD, counts as the one unit it is.
 * OUTPUTS.  d_out_ids / d_out_offsets (n_docs + 1 entries) are EXACTLY what the matching encode entry writes for the same arguments -- tkz_encode_batch_special_*
 * when n_allowed > 0 and literals are registered, the plain entry otherwise; the ids go straight into the caller's buffer.
 *   doc_chunk_offsets (n_docs + 1 entries)   the chunks of document d are [doc_chunk_offsets[d], doc_chunk_offsets[d + 1]);
 *   chunk_tokens (chunk_cap + 1 entries)     entry c is the index in out_ids of chunk c's first token, entry n_chunks the token total: chunk c is the ids
 *                                            [chunk_tokens[c], chunk_tokens[c + 1]);
 *   chunk_bytes, chunk_units (chunk_cap entries each, int64; either or both may be NULL)   the chunk's start relative to ITS DOCUMENT.  A chunk ends where the next
 *                                            chunk of its document starts, or at the document's length.  The positions are 64-bit: the span entries' limit of 2^31
 *                                            bytes a document does not apply.
 * CAPACITY.  TKZ_E_CAPACITY when out_cap or chunk_cap is short: *total_tokens and *n_chunks then hold the required sizes, nothing is promised in the outputs.
 * A document of t tokens has at most 2 * t / max_tokens + 1 chunks (two consecutive chunks hold more than max_tokens tokens together), and a token is at least a
 * byte: n_docs + 2 * total_bytes / max_tokens chunks ALWAYS suffice (and total_bytes ids).
 *   tkz_encode_batch_chunks_device: device buffers.  Everything else -- allowed / n_allowed, TKZ_E_ARG, TKZ_E_UNSUPPORTED, tkz_encoder_special_stats, device-side
 *     errors, retries inside the call, workspace growth -- as tkz_encode_batch_spans_device; an empty batch clears d_out_offsets and d_doc_chunk_offsets on the
 *     stream (and sets chunk_tokens[0] = 0).  The launch sequence is the piece-granular one of the trim entry (it waits once, inside, for the number of pieces);
 *     behind it the documents are walked twice -- count (k_chunk_walk, k_chunk_walk_long), scan, write -- and, with d_chunk_units, k_chunk_unitcount, a scan and
 *     k_chunk_units.  Workspace beyond the trim entry's piece arrays: 24 bytes a document, and with d_chunk_units 12 bytes per 128 bytes of text.
 *     SERIAL LIMITS.  A document of at most 1,024 items is walked by ONE lane, a galloping search a chunk.  A longer one is walked by ONE wavefront: its chunks are a
 *     chain, each starts where the one before ended, so one document of many megabytes costs a step a chunk and a load per 64 items on that wavefront -- the walk
 *     is not split inside a document.  The bytes of an item over the budget are found by ONE lane that walks the item's ids: an item of many megabytes is walked
 *     by one lane, as in the span entries.
 *   tkz_encode_batch_chunks_utf8: host buffers.  The WHOLE batch is staged, ONE call of the device entry, the results downloaded, as tkz_encode_batch_spans_utf8:
 *     no chunk pipeline, no single-launch route.  *needed_ids / *needed_chunks: the counts, the required ones on TKZ_E_CAPACITY.
 *   tkz_encode_batch_chunks_utf16: code units in, transcoded on the device as tkz_encode_batch_trim_utf16; unit_offsets and chunk_units in code units.  There is no
 *     chunk_bytes: the bytes never exist on the host.  Literals that hold U+FFFD as in the other UTF-16 special entries.
 *   tkz_encode_chunks_utf8 / _utf16: ONE text -- the batch entry with one document, at every size.  TKZ_E_ARG for a negative len or a null n_out / n_chunks.
 * These entries have no overlap between chunks (the overlap entries below do).  There is no budget per document, no _begin / _end form and no form that returns
 * the boundaries without the ids. */
tkz_status tkz_encode_batch_chunks_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                          const int32_t* allowed, int32_t n_allowed, int64_t max_tokens, int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets,
                                          int64_t* d_doc_chunk_offsets, int64_t* d_chunk_tokens, int64_t* d_chunk_bytes, int64_t* d_chunk_units, int64_t chunk_cap,
                                          void* hip_stream, int64_t* total_tokens, int64_t* n_chunks);
tkz_status tkz_encode_batch_chunks_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                        int64_t max_tokens, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* doc_chunk_offsets, int64_t* chunk_tokens,
                                        int64_t* chunk_bytes, int64_t* chunk_units, int64_t chunk_cap, int64_t* needed_ids, int64_t* needed_chunks);
tkz_status tkz_encode_batch_chunks_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                         int64_t max_tokens, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* doc_chunk_offsets, int64_t* chunk_tokens,
                                         int64_t* chunk_units, int64_t chunk_cap, int64_t* needed_ids, int64_t* needed_chunks);
tkz_status tkz_encode_chunks_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t max_tokens, int32_t* out_ids,
                                  int64_t out_cap, int64_t* chunk_tokens, int64_t* chunk_bytes, int64_t* chunk_units, int64_t chunk_cap, int64_t* n_out, int64_t* n_chunks);
tkz_status tkz_encode_chunks_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t max_tokens, int32_t* out_ids,
                                   int64_t out_cap, int64_t* chunk_tokens, int64_t* chunk_units, int64_t chunk_cap, int64_t* n_out, int64_t* n_chunks);
/* informational: successful calls of the chunk entries */
void tkz_encoder_chunks_calls(const tkz_encoder* e, int64_t* calls);

/* ---- Overlapping token-budget chunks: the chunk entries with a second number, as every text splitter takes -- a chunk size and an overlap ----
 * max_tokens = N >= 1 and overlap = O with 0 <= O < N; anything else is TKZ_E_ARG, in every entry.  Items, T (the document's tokens) and "item boundary" are
 * those of the chunk rule above.
 *   - chunk c is the ids [s_c, e_c); s_0 is the document's first token;
 *   - e_c is the chunk rule's end for a chunk that starts at s_c: T when T - s_c <= N; else the largest item boundary b with s_c < b <= s_c + N; else s_c + N,
 *     inside the item;
 *   - the chunk with e_c == T is the document's last;
 *   - otherwise let x = max(e_c - O, s_c + 1): s_{c+1} is the smallest item boundary b with x <= b <= e_c, and where there is none, s_{c+1} = x (then e_c lies
 *     inside an oversize item, and so does the next start);
 *   - if the chunk so begun would end at e_c again it adds nothing, so s_{c+1} = e_c instead (the item behind e_c is too large for what the overlap left of the
 *     budget).
 * So: O = 0 gives exactly the chunks of the entries above; 1 <= e_c - s_c <= N; s_c < s_{c+1} <= e_c < e_{c+1}; consecutive chunks share e_c - s_{c+1} <= O
 * tokens; s_{c+1} is an item boundary unless e_c is not one; e_{c+2} - e_c > N - O.  While no item exceeds the budget the chunk is EncodeTrimSuffix(rest, N) and
 * the text the next chunk starts with is what EncodeTrimPrefix(chunk text, O) keeps -- when that keeps the whole chunk, the chunk's first item is dropped.
 * TABLE.  The chunks no longer partition the ids:
 *   doc_chunk_offsets (n_docs + 1 entries)   as above;
 *   chunk_tokens (chunk_cap entries)         s_c as an index into out_ids;
 *   chunk_ends (chunk_cap entries, required) e_c as an index into out_ids;
 *   chunk_bytes, chunk_units                 as above: where the chunk's text starts, relative to its document;
 *   chunk_end_bytes, chunk_end_units (chunk_cap entries each, int64; either or both may be NULL)   where the chunk's text ends, relative to its document: the
 *                                            position of token e_c under the same rules, or the document's length in bytes or units for its last chunk.
 * CAPACITY as above, with N - O in the place of N: a document of t tokens has at most 2 * t / (N - O) + 1 chunks, n_docs + 2 * total_bytes / (N - O) chunks ALWAYS
 * suffice, and never more than a chunk a token (the starts ascend strictly).
 * out_ids, out_offsets, allowed / n_allowed, the error codes, the empty batch (d_out_offsets and d_doc_chunk_offsets cleared; the table arrays are not touched)
 * and the host entries' staging are those of the matching chunk entry.  The launch sequence is the chunk entries' with walks of its own (k_chunkov_walk,
 * k_chunkov_walk_long) and k_chunkov_units for both unit arrays; the unit stage runs when either is given.  The serial limits are the chunk entries'; the start
 * search adds a binary search over the chunk's items (lane walk) or a load of 64 items per 64 items of overlap (wavefront walk) to every chunk.
 * There is no overlap or budget per document, no _begin / _end form and no form that returns the boundaries without the ids. */
tkz_status tkz_encode_batch_chunks_overlap_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                                  const int32_t* allowed, int32_t n_allowed, int64_t max_tokens, int64_t overlap, int32_t* d_out_ids, int64_t out_cap,
                                                  int64_t* d_out_offsets, int64_t* d_doc_chunk_offsets, int64_t* d_chunk_tokens, int64_t* d_chunk_ends,
                                                  int64_t* d_chunk_bytes, int64_t* d_chunk_units, int64_t* d_chunk_end_bytes, int64_t* d_chunk_end_units,
                                                  int64_t chunk_cap, void* hip_stream, int64_t* total_tokens, int64_t* n_chunks);
tkz_status tkz_encode_batch_chunks_overlap_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed,
                                                int32_t n_allowed, int64_t max_tokens, int64_t overlap, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                                int64_t* doc_chunk_offsets, int64_t* chunk_tokens, int64_t* chunk_ends, int64_t* chunk_bytes, int64_t* chunk_units,
                                                int64_t* chunk_end_bytes, int64_t* chunk_end_units, int64_t chunk_cap, int64_t* needed_ids, int64_t* needed_chunks);
tkz_status tkz_encode_batch_chunks_overlap_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed,
                                                 int32_t n_allowed, int64_t max_tokens, int64_t overlap, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                                 int64_t* doc_chunk_offsets, int64_t* chunk_tokens, int64_t* chunk_ends, int64_t* chunk_units, int64_t* chunk_end_units,
                                                 int64_t chunk_cap, int64_t* needed_ids, int64_t* needed_chunks);
tkz_status tkz_encode_chunks_overlap_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t max_tokens,
                                          int64_t overlap, int32_t* out_ids, int64_t out_cap, int64_t* chunk_tokens, int64_t* chunk_ends, int64_t* chunk_bytes,
                                          int64_t* chunk_units, int64_t* chunk_end_bytes, int64_t* chunk_end_units, int64_t chunk_cap, int64_t* n_out, int64_t* n_chunks);
tkz_status tkz_encode_chunks_overlap_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t max_tokens,
                                           int64_t overlap, int32_t* out_ids, int64_t out_cap, int64_t* chunk_tokens, int64_t* chunk_ends, int64_t* chunk_units,
                                           int64_t* chunk_end_units, int64_t chunk_cap, int64_t* n_out, int64_t* n_chunks);
/* informational: successful calls of the overlap chunk entries */
void tkz_encoder_chunks_overlap_calls(const tkz_encoder* e, int64_t* calls);

/* ---- Packed rows: BOS / EOS framing, rows of the context length, positions and segment starts, in ONE call ----
 * What a corpus-tokenisation job does next with the ragged result: an end-of-text id behind (or a begin id in front of) every document, the stream laid out as rows
 * of the context length, the tail padded, and the two things a packed-sequence attention kernel needs -- a position that restarts at every document and the list of
 * segment starts (cu_seqlens).
 * THE RULE.  Let ids / O[0..n_docs] be EXACTLY what the matching encode entry writes for the same arguments -- tkz_encode_batch_special_* when n_allowed > 0 and
 * literals are registered, the plain entry otherwise.
 *   Parameters.  bos_id, eos_id: -1 means none, any value >= 0 is taken as it is (it need not be in the vocabulary), < -1 is TKZ_E_ARG.  fb = bos_id >= 0,
 *     fe = eos_id >= 0, f = fb + fe.  row_len = L with 1 <= L <= 2^31 - 1, anything else is TKZ_E_ARG.  pad_id: any int32.
 *   Stream.  For every document in order, empty ones included: [bos_id] if fb, then the document's ids, then [eos_id] if fe.  Document d starts at stream index
 *     s[d] = O[d] + f * d; the stream has T = O[n_docs] + f * n_docs entries.  Documents are never reordered, dropped or truncated.
 *   Rows.  n_rows = ceil(T / L).  out_ids[t] = stream[t] for t < T, and pad_id for T <= t < n_rows * L.  Nothing at or behind n_rows * L is touched.
 *   Offsets.  out_offsets[d] = s[d] (n_docs + 1 entries, the last is T).
 *   Segments.  t < T is a segment start iff t % L == 0, or t == s[d] for a document with s[d + 1] > s[d].  A document start on a row boundary is ONE segment
 *     start.  seg_starts holds them ascending, n_segs of them, and seg_starts[n_segs] = T.  Always n_segs <= n_rows + n_docs.
 *   Positions.  pos[t] = t - (largest segment start <= t) for t < T, and 0 for the padding.  So 0 <= pos[t] < L.
 *   Example: documents [a1 a2 a3], [], [c1 c2], no bos, eos = E.  s = 0,4,5,8 and T = 8.
 *     L = 4: rows a1 a2 a3 E / E c1 c2 E;        seg_starts 0,4,5,8 (n_segs 3);      pos 0,1,2,3,0,0,1,2
 *     L = 3: rows a1 a2 a3 / E E c1 / c2 E pad;  seg_starts 0,3,4,5,6,8 (n_segs 5);  pos 0,1,2,0,0,0,0,1,0
 * CAPACITY.  TKZ_E_CAPACITY when out_cap < n_rows * L, or when d_seg_starts != NULL && seg_cap < n_segs.  *total_tokens (T), *n_rows and *n_segs then hold the
 * required figures, all three from the one call; nothing is promised in the outputs.  *n_segs is reported whether or not d_seg_starts is given.  Sizes that
 * ALWAYS suffice (a token is at least a byte): ids -- and pos -- (total_bytes + f * n_docs) rounded up to a multiple of L (UTF-16: 3 * units for the bytes);
 * segments n_docs + ceil((total_bytes + f * n_docs) / L), and one more entry for seg_starts[n_segs].
 *   tkz_encode_batch_packed_device: device buffers.  d_pos (out_cap entries) and d_seg_starts (seg_cap + 1 entries) may each be NULL; total_tokens, n_rows and
 *     n_segs may not (TKZ_E_ARG).  Everything else -- allowed / n_allowed, TKZ_E_ARG, TKZ_E_UNSUPPORTED, tkz_encoder_special_stats, device-side errors, retries
 *     inside the call, workspace growth, returning after the stream has drained -- as tkz_encode_batch_spans_device.  Nothing is read outside
 *     d_bytes[0, total_bytes), nothing is written at or behind n_rows * L (ids, pos), seg_cap + 1 (seg_starts) or n_docs + 1 (offsets).  An empty batch
 *     (n_docs == 0) is TKZ_OK: the offsets cleared on the stream, seg_starts[0] = 0, all three counts 0; documents that are all empty still have a stream when
 *     f > 0 (T = f * n_docs).  The encoder's {n_docs, n_bytes, n_tokens} block (and a count block where one is given) receives T.
 *     The launch sequence is the PLAIN document-granular one of tkz_encode_batch_device -- no piece arrays, no wait for a piece count.  With f == 0 the ids are
 *     written straight into d_out_ids as that entry writes them and are not moved again; with f > 0 the unframed ids and offsets stay in the workspace (4 bytes per
 *     input byte, 8 per document) and the stage gathers them into the caller's buffer.  The stage: k_pack_count (segment starts per tile of 2,048 stream
 *     positions), the scan of the counts, k_pack_write.  Workspace of the stage: 12 bytes per tile.
 *   tkz_encode_batch_packed_utf8: host buffers.  The WHOLE batch is staged, ONE call of the device entry, the results downloaded, as tkz_encode_batch_spans_utf8:
 *     no chunk pipeline, no single-launch route.  pos (out_cap entries) and seg_starts (seg_cap + 1) may be NULL, total_tokens too; *needed_ids = n_rows * L and
 *     *needed_segs = n_segs, the required ones on TKZ_E_CAPACITY (both pointers are required).
 *   tkz_encode_batch_packed_utf16: code units in, transcoded on the device as tkz_encode_batch_spans_utf16; unit_offsets in code units.
 * There is no best-fit packing (documents keep their order and are cut at row ends), no per-token document index, no per-document truncation (trim first), no
 * _begin / _end form and no single-text form (packing one text is a reshape). */
tkz_status tkz_encode_batch_packed_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                          const int32_t* allowed, int32_t n_allowed, int32_t bos_id, int32_t eos_id, int64_t row_len, int32_t pad_id,
                                          int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets, int32_t* d_pos, int64_t* d_seg_starts, int64_t seg_cap,
                                          void* hip_stream, int64_t* total_tokens, int64_t* n_rows, int64_t* n_segs);
tkz_status tkz_encode_batch_packed_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                        int32_t bos_id, int32_t eos_id, int64_t row_len, int32_t pad_id, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                        int32_t* pos, int64_t* seg_starts, int64_t seg_cap, int64_t* total_tokens, int64_t* needed_ids, int64_t* needed_segs);
tkz_status tkz_encode_batch_packed_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                         int32_t bos_id, int32_t eos_id, int64_t row_len, int32_t pad_id, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                         int32_t* pos, int64_t* seg_starts, int64_t seg_cap, int64_t* total_tokens, int64_t* needed_ids, int64_t* needed_segs);
/* informational: successful calls of the packed entries */
void tkz_encoder_packed_calls(const tkz_encoder* e, int64_t* calls);

/* ---- Padded rows: one row a document, cut to a maximum length, framed, padded to a common width, with the attention mask, in ONE call ----
 * The inference half of what follows an encode call (packed rows above are the training half): tokenizer(texts, truncation=True, padding=True, max_length=L,
 * pad_to_multiple_of=M) -- what a prefill, embedding or reranker batch and an evaluation harness need before the model can run.
 * THE RULE.  Let ids / O[0..n_docs] be EXACTLY what the matching encode entry writes for the same arguments -- tkz_encode_batch_special_* when n_allowed > 0 and
 * literals are registered, the plain entry otherwise.  n[d] = O[d + 1] - O[d].
 *   Parameters.  bos_id, eos_id: as in the packed entries: -1 means none, any value >= 0 is taken as it is, < -1 is TKZ_E_ARG; fb = bos_id >= 0, fe = eos_id >= 0,
 *     f = fb + fe.  max_len = L with max(1, f) <= L <= 2^31 - 1, anything else is TKZ_E_ARG.  cut_side: a tkz_trim_side -- TKZ_TRIM_SUFFIX cuts the end and keeps
 *     the head, TKZ_TRIM_PREFIX cuts the front and keeps the tail.  pad_side: TKZ_PAD_RIGHT or TKZ_PAD_LEFT.  Any other side value is TKZ_E_ARG.  pad_id: any
 *     int32.  pad_multiple = M with 0 <= M <= 2^31 - 1, anything else is TKZ_E_ARG.
 *   Cut (token-granular).  k[d] = min(n[d], L - f) ids are kept: ids[O[d] .. O[d] + k[d]) for the suffix cut, ids[O[d + 1] - k[d] .. O[d + 1]) for the prefix
 *     cut.  The framing is added AFTER the cut, so it always survives: len[d] = k[d] + f, and an empty document is its framing alone.  n_cut is the number of
 *     documents with n[d] > L - f.  This is a plain cut of the id list, as truncation=True makes it; it is NOT the reference's whole-item cut
 *     (EncodeTrimSuffix / EncodeTrimPrefix keep or drop a pre-tokenizer piece as a whole): tkz_encode_batch_trim_* remains for that.
 *   Width.  M == 0: W = L, a fixed width.  M >= 1: W = min(L, ceil(max_d len[d] / M) * M).  W = 0 when n_docs == 0 or every len[d] is 0; nothing is written then.
 *   Rows.  Row d is out[d * W .. (d + 1) * W).  Its content is [bos_id] kept [eos_id], len[d] entries: at columns [0, len[d]) with pad_id behind it for
 *     TKZ_PAD_RIGHT, at columns [W - len[d], W) with pad_id in front of it for TKZ_PAD_LEFT.  mask (uint8; it views as bool): 1 on content, 0 on padding.
 *     pos (int32): the index inside the content, 0 .. len[d] - 1, and 0 on padding.  lens[d] = len[d] (int32).  out_offsets[d] = O[d] (int64, n_docs + 1
 *     entries): the UNCUT offsets, so n[d] - (lens[d] - f) is what was cut.
 *   Scalars.  *total_tokens = O[n_docs], the uncut total -- which is also what the encoder's {n_docs, n_bytes, n_tokens} block receives --, *width = W, *n_cut.
 *   Example: documents [a1 a2 a3 a4 a5], [], [c1 c2]; bos = B, no eos, L = 4, M = 1, pad P.  W = 4, lens = 4, 1, 3, n_cut = 1.
 *     suffix cut, right pad: rows B a1 a2 a3 / B P P P / B c1 c2 P;  pos 0 1 2 3 / 0 0 0 0 / 0 1 2 0;  mask 1111 / 1000 / 1110
 *     prefix cut, left pad:  rows B a3 a4 a5 / P P P B / P B c1 c2;  pos 0 1 2 3 / 0 0 0 0 / 0 0 1 2;  mask 1111 / 0001 / 0111
 * CAPACITY.  TKZ_E_CAPACITY when out_cap < n_docs * W.  *width, *total_tokens and *n_cut then hold the required figures, all from the one call; nothing is
 * promised in the outputs.  n_docs * L entries ALWAYS suffice.
 *   tkz_encode_batch_padded_device: device buffers.  d_mask (out_cap bytes), d_pos (out_cap entries) and d_out_offsets (n_docs + 1) may each be NULL; d_out_ids
 *     (out_cap entries), d_lens (n_docs entries), total_tokens, width and n_cut may not (TKZ_E_ARG).  Everything else -- allowed / n_allowed, TKZ_E_UNSUPPORTED,
 *     tkz_encoder_special_stats, device-side errors, retries of an attempt inside the call, workspace growth, returning after the stream has drained -- as
 *     tkz_encode_batch_packed_device.  Nothing is read outside d_bytes[0, total_bytes), nothing is written at or behind n_docs * W (ids, mask, pos), n_docs (lens)
 *     or n_docs + 1 (offsets); an attempt that is run again inside the call has written nothing into the caller's buffers.  An empty batch (n_docs == 0) is
 *     TKZ_OK: out_offsets[0] cleared on the stream, all three scalars 0.
 *     The launch sequence is the PLAIN document-granular one of tkz_encode_batch_device -- no piece arrays, no wait for a piece count.  The uncut ids and offsets
 *     stay in the workspace (4 bytes per input byte, 8 per document), as a framed packed call keeps them.  The stage: k_pad_lens (a lane a document: lens, the
 *     first kept id of every document -- 8 bytes per document of workspace --, and the longest row and the cut documents of every workgroup), then k_pad_write
 *     (the width from those partials, the capacity check on the device, the rows by output position in tiles of 1,024).  The host does not wait between the two.
 *   tkz_encode_batch_padded_utf8: host buffers.  The WHOLE batch is staged, ONE call of the device entry, the results downloaded, as
 *     tkz_encode_batch_packed_utf8: no chunk pipeline, no single-launch route.  mask, pos and out_offsets may be NULL.  Only the rows, the mask, pos, lens and the
 *     offsets are downloaded, NEVER the uncut ids: a batch cut to L moves n_docs * W ids over PCIe where tkz_encode_batch_utf8 moves total_tokens -- on long
 *     documents that download is what bounds the host entries.
 *   tkz_encode_batch_padded_utf16: code units in, transcoded on the device as tkz_encode_batch_packed_utf16; unit_offsets in code units.
 * There is no item-granular cut in front of the rows (trim first), no maximum per document, no sorting or bucketing by length HERE (the bucketed entries below do
 * that), no _begin / _end form, no chunk
 * pipeline, no single-text form (padding one text is a slice) and no int64 or bool mask. */
typedef enum tkz_pad_side { TKZ_PAD_RIGHT = 0, TKZ_PAD_LEFT = 1 } tkz_pad_side;
tkz_status tkz_encode_batch_padded_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                          const int32_t* allowed, int32_t n_allowed, int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side,
                                          int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int32_t* d_out_ids, int64_t out_cap, uint8_t* d_mask,
                                          int32_t* d_pos, int32_t* d_lens, int64_t* d_out_offsets, void* hip_stream, int64_t* total_tokens, int64_t* width,
                                          int64_t* n_cut);
tkz_status tkz_encode_batch_padded_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                        int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                        int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos, int32_t* lens, int64_t* out_offsets,
                                        int64_t* total_tokens, int64_t* width, int64_t* n_cut);
tkz_status tkz_encode_batch_padded_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                         int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                         int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos, int32_t* lens, int64_t* out_offsets,
                                         int64_t* total_tokens, int64_t* width, int64_t* n_cut);
/* informational: successful calls of the padded entries */
void tkz_encoder_padded_calls(const tkz_encoder* e, int64_t* calls);

/* ---- Length-bucketed padded rows: the documents sorted by token length, cut into mini-batches of B rows, every mini-batch padded to ITS OWN longest row ----
 * What follows the padded rows above in every inference and evaluation loop (group_by_length, a length-sorted sampler, a sorted prefill queue): sort by length,
 * cut the sorted list into buckets, pad each bucket alone, keep the permutation.  The lengths exist on the device only after the encode; this is that step there.
 * THE RULE.  Every argument of tkz_encode_batch_padded_device keeps its meaning and its TKZ_E_ARG conditions: allowed / n_allowed, bos_id, eos_id, max_len = L,
 * cut_side, pad_side, pad_id, pad_multiple = M.  Two more: bucket_rows = B with 1 <= B <= 2^31 - 1, and order, a tkz_bucket_order; anything else is TKZ_E_ARG.
 *   Lengths.  n[d], k[d] = min(n[d], L - f), len[d] = k[d] + f and n_cut are EXACTLY as in the padded rule: the same cut, the framing after the cut.
 *   Order.  order[0 .. n_docs) (int64) is the permutation of the documents by len, ascending or descending as asked; documents of equal len keep ascending
 *     document index in BOTH directions: ascending is numpy.argsort(len, kind="stable"), descending is numpy.argsort(-len, kind="stable").  rank[d] (int64,
 *     optional) is the inverse: rank[order[r]] = r.
 *   Buckets.  n_buckets = ceil(n_docs / B) -- the caller computes it before the call, so there is no bucket capacity argument.  Bucket b holds the sorted rows
 *     [b * B, min((b + 1) * B, n_docs)): R_b rows.  maxlen_b is the largest len in the bucket.  M == 0: W_b = L.  M >= 1: W_b = min(L, ceil(maxlen_b / M) * M).
 *     W_b = 0 when maxlen_b == 0.  bucket_widths[b] = W_b (int32, n_buckets entries).  bucket_offsets[b] = the sum over b' < b of R_b' * W_b' (int64,
 *     n_buckets + 1 entries); the last entry is P, the total number of positions.
 *   Rows.  Sorted row r lies in bucket b = r / B as row i = r - b * B and occupies out[bucket_offsets[b] + i * W_b .. + W_b).  Its content is the padded rule's
 *     row for document order[r] at width W_b: [bos_id] kept [eos_id] on the side pad_side says, pad_id elsewhere; mask (uint8) 1 on content; pos (int32) the
 *     index inside the content, 0 on padding.  lens[d] (int32) and out_offsets[d] (int64, UNCUT) stay in DOCUMENT order, as in the padded entry.
 *   Scalars.  *total_tokens = O[n_docs], the uncut total -- which is also what the encoder's {n_docs, n_bytes, n_tokens} block receives --, *total_positions = P,
 *     *n_cut.
 *   Example: documents [a1 a2 a3 a4 a5], [], [c1 c2], [d1 d2 d3], [e1 e2]; no bos, eos = X, L = 4, M = 1, B = 2, pad P, suffix cut, right padding.
 *     len = 4, 1, 3, 4, 3; n_cut = 1.
 *     ascending:  order 1, 2, 4, 0, 3; rank 3, 0, 1, 4, 2; widths 3, 4, 4; bucket offsets 0, 6, 14, 18; P = 18
 *                 rows X P P / c1 c2 X | e1 e2 X P / a1 a2 a3 X | d1 d2 d3 X
 *     descending: order 0, 3, 2, 4, 1; rank 0, 4, 2, 1, 3; widths 4, 3, 1; bucket offsets 0, 8, 14, 15; P = 15
 *                 rows a1 a2 a3 X / d1 d2 d3 X | c1 c2 X / e1 e2 X | X
 *     The padded entry writes 20 positions for the same batch.
 * CAPACITY.  TKZ_E_CAPACITY when out_cap < P.  *total_tokens, *total_positions and *n_cut then hold the required figures, all from the one call; nothing is
 * promised in the outputs.  n_docs * L entries ALWAYS suffice.
 *   tkz_encode_batch_bucketed_device: device buffers.  d_mask (out_cap bytes), d_pos (out_cap entries), d_out_offsets (n_docs + 1) and d_rank (n_docs) may each be
 *     NULL; d_out_ids (out_cap entries), d_lens and d_order (n_docs entries), d_bucket_offsets (n_buckets + 1), d_bucket_widths (n_buckets) and the three scalars
 *     may not (TKZ_E_ARG).  Nothing is written at or behind P (ids, mask, pos), n_docs (lens, order, rank), n_docs + 1 (offsets), n_buckets (widths) or
 *     n_buckets + 1 (bucket offsets).  An empty batch (n_docs == 0) is TKZ_OK: bucket_offsets[0] and out_offsets[0] cleared on the stream, all three scalars 0.
 *     Everything else -- special tokens, TKZ_E_UNSUPPORTED, device-side errors, an attempt that is run again inside the call writing nothing of the caller's,
 *     workspace growth, returning after the stream has drained -- as tkz_encode_batch_padded_device.
 *     The launch sequence is the padded call's up to and including k_pad_lens, unchanged.  Then, without a host wait: a stable LSD radix sort of (len, document)
 *     -- 8 bits a pass, as many passes as the bytes L occupies (L = 512: two), k_bkt_hist, a scan and k_bkt_scatter each; 36 bytes of workspace a document --,
 *     k_bkt_table (W_b and R_b * W_b; maxlen_b is the bucket's first or last sorted row), a 64-bit scan (the offsets and P), and k_bkt_write (the capacity check
 *     on the device, the rows by output position in tiles of 1,024 with the width looked up per bucket).
 *   tkz_encode_batch_bucketed_utf8: host buffers.  The WHOLE batch is staged, ONE call of the device entry, the results downloaded, as
 *     tkz_encode_batch_padded_utf8.  mask, pos, out_offsets and rank may be NULL.  The rows (P positions), the mask, pos, lens, order, rank, the bucket arrays and
 *     the offsets are downloaded, NEVER the uncut ids.
 *   tkz_encode_batch_bucketed_utf16: code units in, transcoded on the device as tkz_encode_batch_padded_utf16; unit_offsets in code units.
 * There is no bucketing by a TOKEN budget HERE (rows * width <= T: the budgeted entries below do that, with bucket_rows as a cap), no item-granular
 * cut, no maximum per document, no _begin / _end form, no chunk pipeline for the host entries, no single-text form and no device-resident UTF-16 input. */
typedef enum tkz_bucket_order { TKZ_BUCKET_ASCENDING = 0, TKZ_BUCKET_DESCENDING = 1 } tkz_bucket_order;
tkz_status tkz_encode_batch_bucketed_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                            const int32_t* allowed, int32_t n_allowed, int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side,
                                            int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int64_t bucket_rows, int32_t order, int32_t* d_out_ids,
                                            int64_t out_cap, uint8_t* d_mask, int32_t* d_pos, int32_t* d_lens, int64_t* d_out_offsets, int64_t* d_order,
                                            int64_t* d_rank, int64_t* d_bucket_offsets, int32_t* d_bucket_widths, void* hip_stream, int64_t* total_tokens,
                                            int64_t* total_positions, int64_t* n_cut);
tkz_status tkz_encode_batch_bucketed_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                          int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                          int64_t bucket_rows, int32_t order, int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos, int32_t* lens,
                                          int64_t* out_offsets, int64_t* order_out, int64_t* rank, int64_t* bucket_offsets, int32_t* bucket_widths,
                                          int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut);
tkz_status tkz_encode_batch_bucketed_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                           int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                           int64_t bucket_rows, int32_t order, int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos, int32_t* lens,
                                           int64_t* out_offsets, int64_t* order_out, int64_t* rank, int64_t* bucket_offsets, int32_t* bucket_widths,
                                           int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut);
/* informational: successful calls of the bucketed entries */
void tkz_encoder_bucketed_calls(const tkz_encoder* e, int64_t* calls);

/* ---- Token-budget buckets: the documents sorted by token length, cut into mini-batches of at most T positions (rows * width), every one padded to ITS OWN longest row ----
 * What training and serving loops make of a sorted batch (fairseq's max_tokens / batch_by_size, a token-budget sampler, a prefill queue with a token limit): every
 * mini-batch costs the same memory whatever its row length, where a fixed row count lets the long buckets set the limit and the short ones waste it.
 * THE RULE.  Every argument of tkz_encode_batch_bucketed_device keeps its meaning and its TKZ_E_ARG conditions, with these differences: bucket_rows = B becomes a
 * CAP on the rows of a bucket, 1 <= B <= 2^31 - 1, and 2^31 - 1 means none; token_budget = T with max_len <= T <= 2^62, so a row alone always fits; bucket_cap >= 0,
 * the entries of the caller's bucket arrays.  Anything outside these ranges is TKZ_E_ARG (and so are more than 2^31 - 1 documents).
 *   Lengths, order, rank.  n[d], k[d], len[d], n_cut, order, rank, lens and out_offsets are EXACTLY as in the bucketed rule.
 *   Width of a length.  w(0) = 0.  Otherwise w(l) = L when M == 0 and w(l) = min(L, ceil(l / M) * M) when M >= 1.
 *   Buckets, greedy over the sorted rows.  Bucket 0 starts at sorted row 0.  A bucket that starts at row s ends at the largest e in (s, n_docs] with e - s <= B and
 *     (e - s) * w(longest len in [s, e)) <= T; the longest len is that of row e - 1 ascending and of row s descending.  The next bucket starts at e; n_buckets is
 *     the count.  Rows of width 0 cost nothing against T: only B stops them.
 *   Bucket arrays.  bucket_rows_out[b] (int64, n_buckets + 1 entries) is the first sorted row of bucket b; the last entry is n_docs.  R_b is the difference of
 *     two neighbours.  bucket_widths[b] = W_b (int32, n_buckets entries), the width of the bucket's longest len.  bucket_offsets[b] = the sum over b' < b of
 *     R_b' * W_b' (int64, n_buckets + 1 entries); the last entry is P.
 *   Rows.  Sorted row r of bucket b is row i = r - bucket_rows_out[b] and occupies out[bucket_offsets[b] + i * W_b .. + W_b).  Content, mask and pos are as in the
 *     bucketed rule.
 *   Scalars.  *total_tokens (uncut, and what the encoder's counts block receives), *total_positions = P, *n_cut, *n_buckets.
 *   Example: the bucketed block's five documents, len = 4, 1, 3, 4, 3; no bos, eos = X, L = 4, M = 1, pad P, suffix cut, right padding.
 *     T = 9, no row cap, ascending (order 1, 2, 4, 0, 3): n_buckets = 2; rows 0, 3, 5; widths 3, 4; bucket offsets 0, 9, 17
 *                 rows X P P / c1 c2 X / e1 e2 X | a1 a2 a3 X / d1 d2 d3 X
 *     the same descending (order 0, 3, 2, 4, 1): n_buckets = 2; rows 0, 2, 5; widths 4, 3; bucket offsets 0, 8, 17
 *                 rows a1 a2 a3 X / d1 d2 d3 X | c1 c2 X / e1 e2 X / X P P
 *     T = 9, B = 2, ascending: rows 0, 2, 4, 5; widths 3, 4, 4; bucket offsets 0, 6, 14, 18 -- the bucketed entry's buckets.
 *   With T >= n_docs * L only B binds: the buckets are those of the bucketed entry with the same B, and bucket_rows_out[b] = min(b * B, n_docs).
 * CAPACITY.  TKZ_E_CAPACITY when out_cap < P or bucket_cap < n_buckets.  All four scalars then hold the required figures, all from the one call; nothing is
 * promised in the outputs.  n_docs * L positions and n_docs buckets ALWAYS suffice.
 *   tkz_encode_batch_budgeted_device: device buffers.  d_mask, d_pos, d_out_offsets and d_rank may each be NULL; d_out_ids, d_lens, d_order, d_bucket_offsets and
 *     d_bucket_rows (bucket_cap + 1 entries each), d_bucket_widths (bucket_cap entries) and the four scalars may not (TKZ_E_ARG).  Nothing is written at or behind P
 *     (ids, mask, pos), n_docs (lens, order, rank), n_docs + 1 (offsets), n_buckets (widths) or n_buckets + 1 (bucket offsets, bucket rows); the bucket arrays may
 *     be larger than that.  An empty batch (n_docs == 0) is TKZ_OK: bucket_offsets[0], bucket_rows_out[0] and out_offsets[0] cleared on the stream, all four
 *     scalars 0.  Everything else as tkz_encode_batch_bucketed_device.
 *     The launch sequence is the bucketed call's up to and including the sort's last k_bkt_scatter, unchanged.  Then, without a host wait -- the host never learns
 *     n_buckets before the call ends; its grids and scans are sized from n_docs, bucket_cap and out_cap --: k_tbk_mark twice around a scan (the RUNS of equal
 *     width: at most min(n_docs, ceil(L / M) + 1), 65 at L = 512, M = 8), k_tbk_chain (ONE wavefront; inside a run every bucket has min(B, T / w) rows, so the
 *     chain of dependent bucket ends is walked a run, not a bucket: its steps do not grow with n_buckets), a scan of the buckets a run, k_tbk_table (a lane a
 *     bucket: its run by one search), a 64-bit scan (the offsets) and k_tbk_write (both capacity checks on the device, the bucket arrays, the rows as k_bkt_write
 *     writes them).  Workspace beside the bucketed call's 36 bytes a document: 12 bytes a 64 documents, 56 bytes a run, 28 bytes a bucket of min(n_docs, bucket_cap).
 *     Known limit: with M = 1 and a very large L the runs, and with them the chain's steps, can reach min(n_docs, L).
 *   tkz_encode_batch_budgeted_utf8: host buffers.  The WHOLE batch is staged, ONE call of the device entry, the results downloaded, as
 *     tkz_encode_batch_bucketed_utf8.  The rows (P positions), the optional arrays and the three bucket arrays are downloaded, NEVER the uncut ids.
 *   tkz_encode_batch_budgeted_utf16: code units in, transcoded on the device as tkz_encode_batch_bucketed_utf16; unit_offsets in code units.
 * There is no row-count multiple (required_batch_size_multiple), no shuffling of the buckets, no maximum per document, no budget in UNPADDED tokens, no
 * _begin / _end form, no chunk pipeline for the host entries and no device-resident UTF-16 input. */
tkz_status tkz_encode_batch_budgeted_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                            const int32_t* allowed, int32_t n_allowed, int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side,
                                            int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int64_t token_budget, int64_t bucket_rows, int32_t order,
                                            int32_t* d_out_ids, int64_t out_cap, uint8_t* d_mask, int32_t* d_pos, int32_t* d_lens, int64_t* d_out_offsets,
                                            int64_t* d_order, int64_t* d_rank, int64_t* d_bucket_offsets, int64_t* d_bucket_rows, int32_t* d_bucket_widths,
                                            int64_t bucket_cap, void* hip_stream, int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut, int64_t* n_buckets);
tkz_status tkz_encode_batch_budgeted_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                          int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                          int64_t token_budget, int64_t bucket_rows, int32_t order, int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos,
                                          int32_t* lens, int64_t* out_offsets, int64_t* order_out, int64_t* rank, int64_t* bucket_offsets, int64_t* bucket_rows_out,
                                          int32_t* bucket_widths, int64_t bucket_cap, int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut, int64_t* n_buckets);
tkz_status tkz_encode_batch_budgeted_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                           int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                           int64_t token_budget, int64_t bucket_rows, int32_t order, int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos,
                                           int32_t* lens, int64_t* out_offsets, int64_t* order_out, int64_t* rank, int64_t* bucket_offsets, int64_t* bucket_rows_out,
                                           int32_t* bucket_widths, int64_t bucket_cap, int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut, int64_t* n_buckets);
/* informational: successful calls of the budgeted entries */
void tkz_encoder_budgeted_calls(const tkz_encoder* e, int64_t* calls);

/* ---- Pair rows: one row a PAIR of texts -- [bos] A sep B [eos] --, cut to a maximum length by a strategy, padded to a common width, with mask and type ids, in ONE call ----
 * What a cross-encoder reranker, an NLI or QA evaluation and a prompt / completion fine-tuning set feed the model: tokenizer(text_a, text_b, truncation=...,
 * max_length=L, padding=True) -- the ids, token_type_ids and the attention mask.  How much of either text survives depends on BOTH lengths, which exist only on
 * the device after the encode.
 * THE RULE.  The batch holds n_docs = 2 * n_pairs documents in the usual layout (one buffer, n_docs + 1 offsets): document 2p is the first text A of pair p,
 * document 2p + 1 its second text B.  An odd n_docs is TKZ_E_ARG.  Let ids / O[0..n_docs] be EXACTLY what the matching encode entry writes for these documents --
 * tkz_encode_batch_special_* when n_allowed > 0 and literals are registered, the plain entry otherwise; `allowed` applies to both texts.
 * a[p] = O[2p + 1] - O[2p], b[p] = O[2p + 2] - O[2p + 1].
 *   Parameters.  bos_id, eos_id: as in the padded entries: -1 means none, any value >= 0 is taken as it is, < -1 is TKZ_E_ARG; fb = bos_id >= 0, fe = eos_id >= 0.
 *     sep_count = s in {0, 1, 2}, anything else is TKZ_E_ARG; sep_id >= 0 when s > 0 (-1 or less is TKZ_E_ARG then); it is not read when s == 0.  The framing
 *     count is f = fb + s + fe.  max_len = L with max(1, f) <= L <= 2^31 - 1, anything else is TKZ_E_ARG.  strategy: a tkz_pair_truncation, anything else is
 *     TKZ_E_ARG.  cut_side, pad_side, pad_id and pad_multiple = M: exactly as in the padded entries; ONE cut_side serves both texts.
 *   Cut (token-granular, a plain cut of the id lists).  R = L - f, h = R / 2 rounded down, H = R - h.  The kept counts ka, kb:
 *     TKZ_PAIR_LONGEST_FIRST: while ka + kb > R, remove one id from the longer text, from the SECOND on a tie.  In closed form, which is what the kernel
 *       computes: ka = min(a, max(H, R - b)), kb = min(b, max(h, R - a)).  So a shorter text that fits its half is kept whole, and when both are cut A gets the
 *       odd id.
 *     TKZ_PAIR_ONLY_FIRST: kb = min(b, R), ka = min(a, R - kb): A gives way first, and B is cut only once nothing of A is left.  This is total where
 *       tokenizer(...) gives up (a second text longer than the room is an error there): the row never exceeds L.
 *     TKZ_PAIR_ONLY_SECOND: ka = min(a, R), kb = min(b, R - ka).
 *     TKZ_TRIM_SUFFIX keeps the heads of both texts, TKZ_TRIM_PREFIX their tails.  The framing is added AFTER the cut, so it always survives:
 *     len[p] = ka + kb + f.  n_cut is the number of pairs with a + b > R.
 *   Width.  As the padded rule, with max_p len[p] in place of the longest document: M == 0: W = L; M >= 1: W = min(L, ceil(max_p len[p] / M) * M).  W = 0 when
 *     n_pairs == 0 or every len[p] is 0; nothing is written then.
 *   Rows.  Row p is out[p * W .. (p + 1) * W).  Its content is [bos_id] A-kept sep_id x s B-kept [eos_id], len[p] entries, at columns [0, len[p]) with pad_id
 *     behind it for TKZ_PAD_RIGHT, at columns [W - len[p], W) with pad_id in front of it for TKZ_PAD_LEFT.  mask (uint8): 1 on content, 0 on padding.
 *     type_ids (uint8): 1 on the kept ids of B and on the eos, 0 everywhere else -- bos, A, every separator and the padding are 0: BERT's token_type_ids, and the
 *     loss mask of a prompt / completion pair.  pos (int32): the index inside the content, 0 on padding.  lens[p] = len[p] (int32, n_pairs entries).
 *     kept[2p] = ka, kept[2p + 1] = kb (int32, n_docs entries).  out_offsets[d] = O[d] (int64, n_docs + 1 entries): the UNCUT offsets.
 *   Scalars.  *total_tokens = O[n_docs], the uncut total -- which is also what the encoder's {n_docs, n_bytes, n_tokens} block receives --, *width = W, *n_cut.
 *   Example: pairs ([a1 a2 a3 a4 a5], [b1 b2 b3]) and ([], [d1]); bos C, one separator S, eos E; L = 8, M = 1, pad P, right padding.  f = 3, R = 5, W = 8,
 *     lens = 8, 4, n_cut = 1.
 *     LONGEST_FIRST, suffix cut: rows C a1 a2 a3 S b1 b2 E / C S d1 E P P P P;  kept 3 2 0 1;  types 00000111 / 00110000
 *     LONGEST_FIRST, prefix cut: row 0 C a3 a4 a5 S b2 b3 E
 *     ONLY_FIRST, suffix cut:    row 0 C a1 a2 S b1 b2 b3 E
 *     ONLY_SECOND, suffix cut:   row 0 C a1 a2 a3 a4 a5 S E;  types of row 0 00000001
 * CAPACITY.  TKZ_E_CAPACITY when out_cap < n_pairs * W.  *width, *total_tokens and *n_cut then hold the required figures, all from the one call; nothing is
 * promised in the outputs.  n_pairs * L entries ALWAYS suffice.
 *   tkz_encode_batch_pairs_device: device buffers.  d_mask, d_type_ids (out_cap bytes each), d_pos (out_cap entries), d_kept (n_docs) and d_out_offsets
 *     (n_docs + 1) may each be NULL; d_out_ids (out_cap entries), d_lens (n_pairs entries), total_tokens, width and n_cut may not (TKZ_E_ARG).  Everything else --
 *     allowed / n_allowed, TKZ_E_UNSUPPORTED, tkz_encoder_special_stats, device-side errors, retries of an attempt inside the call (which leave the caller's
 *     buffers untouched), workspace growth, returning after the stream has drained, the empty batch (TKZ_OK, out_offsets[0] cleared, all three scalars 0), failed
 *     calls not being counted -- as tkz_encode_batch_padded_device.  Nothing is written at or behind n_pairs * W (ids, mask, types, pos), n_pairs (lens), n_docs
 *     (kept) or n_docs + 1 (offsets).
 *     The launch sequence is the PLAIN document-granular one; the uncut ids and offsets stay in the workspace (4 bytes per input byte, 8 per document).  The
 *     stage: k_pair_lens (a lane a pair: the two kept counts, lens, the first kept id of either text -- one record of 24 bytes a pair of workspace --, and the longest row and the
 *     cut pairs of every workgroup), then k_pair_write (the width from those partials, the capacity check on the device, the rows by output position in tiles of
 *     1,024).  The host does not wait between the two.
 *   tkz_encode_batch_pairs_utf8: host buffers.  The WHOLE batch is staged, ONE call of the device entry, the results downloaded, as
 *     tkz_encode_batch_padded_utf8.  mask, type_ids, pos, kept and out_offsets may be NULL.  Only the rows, the mask, the types, pos, lens, kept and the offsets
 *     are downloaded, NEVER the uncut ids.
 *   tkz_encode_batch_pairs_utf16: code units in, transcoded on the device as tkz_encode_batch_padded_utf16 (a lone surrogate is U+FFFD); unit_offsets in units.
 * NOT in these entries: an item-granular cut, a maximum per pair, stride or overflowing windows for long second texts, more than two segments a row or templates,
 * bucketing or budgeting of pair rows, _begin / _end halves, a chunk pipeline for the host entries, device-resident UTF-16 input, a single-pair launch, and exact
 * agreement with any other library's tie-breaking: the rule above is the contract. */
typedef enum tkz_pair_truncation { TKZ_PAIR_LONGEST_FIRST = 0, TKZ_PAIR_ONLY_FIRST = 1, TKZ_PAIR_ONLY_SECOND = 2 } tkz_pair_truncation;
tkz_status tkz_encode_batch_pairs_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                         const int32_t* allowed, int32_t n_allowed, int32_t bos_id, int32_t sep_id, int32_t sep_count, int32_t eos_id, int64_t max_len,
                                         int32_t strategy, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int32_t* d_out_ids, int64_t out_cap,
                                         uint8_t* d_mask, uint8_t* d_type_ids, int32_t* d_pos, int32_t* d_lens, int32_t* d_kept, int64_t* d_out_offsets, void* hip_stream,
                                         int64_t* total_tokens, int64_t* width, int64_t* n_cut);
tkz_status tkz_encode_batch_pairs_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                       int32_t bos_id, int32_t sep_id, int32_t sep_count, int32_t eos_id, int64_t max_len, int32_t strategy, int32_t cut_side,
                                       int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int32_t* out_ids, int64_t out_cap, uint8_t* mask, uint8_t* type_ids,
                                       int32_t* pos, int32_t* lens, int32_t* kept, int64_t* out_offsets, int64_t* total_tokens, int64_t* width, int64_t* n_cut);
tkz_status tkz_encode_batch_pairs_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                        int32_t bos_id, int32_t sep_id, int32_t sep_count, int32_t eos_id, int64_t max_len, int32_t strategy, int32_t cut_side,
                                        int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int32_t* out_ids, int64_t out_cap, uint8_t* mask, uint8_t* type_ids,
                                        int32_t* pos, int32_t* lens, int32_t* kept, int64_t* out_offsets, int64_t* total_tokens, int64_t* width, int64_t* n_cut);
/* informational: successful calls of the pair entries */
void tkz_encoder_pairs_calls(const tkz_encoder* e, int64_t* calls);

/* ---- Decode (TikTokenizer.cs:586-604) for a batch ---------------------------------------------
 * Document d of the result is the concatenation of the byte strings of ids[id_offsets[d] .. id_offsets[d+1]): a vocabulary id
 * yields its key, a registered special token its UTF-8 literal, any other id nothing (the reference drops unknown ids silently,
 * :591-599).  The bytes are what the reference hands to Encoding.UTF8.GetString; the string conversion is the host's.
 * tkz_encoder_set_special_tokens registers SpecialTokensDecoder (TikTokenizer.cs:79): literal i = literals_utf8[literal_offsets[i]
 * .. literal_offsets[i+1]) for id ids[i] (a vocabulary id is never shadowed, :591-598).  out_cap too small: TKZ_E_CAPACITY and
 * the required byte count in *total_bytes / *needed. */
tkz_status tkz_encoder_set_special_tokens(tkz_encoder* e, const int32_t* ids, const uint8_t* literals_utf8, const int64_t* literal_offsets, int32_t n);
tkz_status tkz_decode_batch_device(tkz_encoder* e, const int32_t* d_ids, const int64_t* d_id_offsets, int64_t n_docs, int64_t total_ids,
                                   uint8_t* d_out_bytes, int64_t out_cap, int64_t* d_out_offsets, void* hip_stream, int64_t* total_bytes);
tkz_status tkz_decode_batch(tkz_encoder* e, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs, uint8_t* out_bytes, int64_t out_cap,
                            int64_t* out_offsets, int64_t* needed);
/* The same with the second half of Decode, Encoding.UTF8.GetString (:603), done on the device: document d of the result is the UTF-16 string of those bytes,
 * out_cap and the offsets count CODE UNITS.  The rule is .NET Core 3.0+'s and WHATWG TextDecoder("utf-8")'s (Unicode 3.9, table 3-7): a well-formed sequence
 * is one unit (a 4-byte one a surrogate pair), every MAXIMAL SUBPART of an ill-formed sequence -- the longest prefix of a well-formed sequence that is present,
 * or one byte -- is one U+FFFD: F0 90 41 -> FFFD 0041, E0 80 -> FFFD FFFD, ED A0 80 and F4 90 80 80 -> one FFFD per byte, C0 / C1 / F5..FF / a stray 80..BF ->
 * one FFFD each.  Every document is decoded on its own: a sequence cut by a document boundary is a prefix (one FFFD) and stray continuation bytes (one each).
 * The units are well-formed UTF-16.  out_cap too small: TKZ_E_CAPACITY and the exact unit total in *total_units / *needed (the bytes of the batch are always
 * sufficient: a unit stands for at least one byte); bad id offsets: TKZ_E_ARG; no ids: offsets of zero.  The call waits once, inside, for the byte total of the
 * batch -- the intermediate bytes live in the workspace and are sized from it (1 byte + 1/8 per decoded byte, 4.25 per 16 for the counts) -- and returns after
 * the stream has drained.  tkz_decode_batch_utf16 stages the whole batch: one upload, one call of the device entry, one download. */
tkz_status tkz_decode_batch_utf16_device(tkz_encoder* e, const int32_t* d_ids, const int64_t* d_id_offsets, int64_t n_docs, int64_t total_ids,
                                         uint16_t* d_out_units, int64_t out_cap, int64_t* d_out_offsets, void* hip_stream, int64_t* total_units);
tkz_status tkz_decode_batch_utf16(tkz_encoder* e, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs, uint16_t* out_units, int64_t out_cap,
                                  int64_t* out_offsets, int64_t* needed);
/* ITokenizer.Decode(int[] tokens) -- ONE id list, as a host calls it after every generation and a streaming host after every few tokens.  The bytes / code units
 * are exactly those of tkz_decode_batch / tkz_decode_batch_utf16 for the same ids as one document.  A list of at most 32,768 ids that decodes to at most 131,072
 * bytes runs as ONE kernel launch on page-locked memory (k_dec_small: no copy commands, one wait), counted by tkz_encoder_small_decode_calls; a longer list, one
 * the kernel hands back (more bytes than that: the second figure of that counter), a device whose LDS per workgroup does not hold the single-launch kernels' and a
 * call with profiling on take the batch entry's path with identical results.  n_ids == 0: TKZ_OK, *n_out = 0, nothing is launched.  TKZ_E_ARG: a null encoder, a
 * null n_out, a negative n_ids or out_cap, null ids with n_ids > 0, a null output with out_cap > 0.  out_cap too small: TKZ_E_CAPACITY and the exact required
 * total in *n_out (bytes / code units), on either route; nothing is promised about the output buffer then. */
tkz_status tkz_decode_utf8(tkz_encoder* e, const int32_t* ids, int64_t n_ids, uint8_t* out_bytes, int64_t out_cap, int64_t* n_out);
tkz_status tkz_decode_utf16(tkz_encoder* e, const int32_t* ids, int64_t n_ids, uint16_t* out_units, int64_t out_cap, int64_t* n_out);
/* Informational: how many single decode calls took the launch, and how many of those the kernel handed back to the batch path.  (Its own counter: the figures
 * of tkz_encoder_small_path_calls count encode calls only.) */
void tkz_encoder_small_decode_calls(const tkz_encoder* e, int64_t* calls, int64_t* handed_back);
/* development: the shader-clock stamps the last k_dec_small left at the end of each of its phases (16 values, 0 where the form has no such phase; returns how many) */
int32_t tkz_encoder_small_decode_phases(const tkz_encoder* e, int64_t* clocks16);

/* ---- token shard files -------------------------------------------------------
 * The on-disk form of one rank's EncodeBatch result: a 64-byte header ("TKZSHRD1", version, n_docs, n_tokens, doc_base,
 * token_base), then offsets int64[n_docs + 1] (relative to the shard), then ids int32[n_tokens]; little-endian.  The
 * reference has no batch or file format (it returns List<int>), so there is nothing to be compatible with.  doc_base /
 * token_base are this rank's bases from tkz_shard_bases: the files of all ranks concatenate into the global result.
 * The device form streams straight from HBM through page-locked chunks (copy of chunk k+1 overlaps the write of chunk k). */
tkz_status tkz_shard_write(const char* path, const int32_t* ids, int64_t n_tokens, const int64_t* offsets, int64_t n_docs,
                           int64_t doc_base, int64_t token_base);
tkz_status tkz_shard_write_device(const char* path, int32_t device, const int32_t* d_ids, int64_t n_tokens, const int64_t* d_offsets,
                                  int64_t n_docs, int64_t doc_base, int64_t token_base);
tkz_status tkz_shard_read_header(const char* path, int64_t* n_docs, int64_t* n_tokens, int64_t* doc_base, int64_t* token_base);

/* ---- multi-GPU ------------------------------------------------------------------------------
 * The reference is single-process; the batch path shards by CONTIGUOUS DOCUMENT RANGES, one process per GPU,
 * vocabulary tables replicated, token ids never leave the GPU that produced them.  The only exchange is ONE all-gather of
 * {n_docs, n_bytes, n_tokens} (3 x int64 per rank) per batch, issued directly on RCCL (ncclAllGather over xGMI) -- no torch,
 * no Python needed in the host.  RCCL is bound at run time (dlopen of librccl.so.1): without it tkz_comm_unique_id /
 * tkz_comm_create fail with TKZ_E_UNSUPPORTED, everything else works.
 *
 *   rank 0:      tkz_comm_unique_id(id)        -> distribute the 128 bytes to the other ranks by any means (file, socket, env)
 *   every rank:  tkz_comm_create(id, rank, world, device, &comm)            (ncclCommInitRank; collective)
 *   per batch:   tkz_shard_range(n_docs_total, rank, world, &lo, &hi); encode documents [lo, hi) on this rank's encoder;
 *                tkz_comm_allgather_counts_device(comm, tkz_encoder_counts_device(enc), d_table, stream)   (asynchronous)
 *             or tkz_comm_allgather_counts(comm, n_docs, n_bytes, n_tokens, table)                          (host, blocking)
 *                tkz_shard_bases(table, world, rank, bases, totals): global index of this shard's first document / byte / token */
typedef struct tkz_comm tkz_comm;
enum { TKZ_COMM_ID_BYTES = 128 };
tkz_status tkz_comm_unique_id(uint8_t* id128);
tkz_status tkz_comm_create(const uint8_t* id128, int32_t rank, int32_t world, int32_t device, tkz_comm** out);
void tkz_comm_destroy(tkz_comm* c);
int32_t tkz_comm_world(const tkz_comm* c);     /* as reported by the communicator (ncclCommCount) */
int32_t tkz_comm_rank(const tkz_comm* c);
const char* tkz_comm_backend(const tkz_comm* c);   /* "rccl <major>.<minor>.<patch>" */
/* d_mine: 3 int64 on the device; d_table: world * 3 int64 on the device (row r = rank r's counts); enqueued on hip_stream */
tkz_status tkz_comm_allgather_counts_device(tkz_comm* c, const int64_t* d_mine, int64_t* d_table, void* hip_stream);
tkz_status tkz_comm_allgather_counts(tkz_comm* c, int64_t n_docs, int64_t n_bytes, int64_t n_tokens, int64_t* table);
/* {n_docs, n_bytes, n_tokens} of the encoder's LAST batch (whichever entry point ran it, the single-launch path included), resident on its
 * device and valid once that batch's stream work is done.  One block per encoder: for callers with one batch at a time.  With several in
 * flight (tkz_encode_batch_device_begin, host threads sharing an encoder) give every batch its own block: tkz_encode_batch_device_begin_counts. */
const int64_t* tkz_encoder_counts_device(const tkz_encoder* e);
/* documents [*lo, *hi) of a job of n_docs_total belong to `rank` */
void tkz_shard_range(int64_t n_docs_total, int32_t rank, int32_t world, int64_t* lo, int64_t* hi);
/* from a gathered table: bases3 = {doc, byte, token} index of this rank's first unit, totals3 = the job totals */
tkz_status tkz_shard_bases(const int64_t* table, int32_t world, int32_t rank, int64_t* bases3, int64_t* totals3);

/* ---- stage-level entry points (used by the parity tests; same kernels as the hot path) --- */

/* Regex.Matches only: writes the piece-start bitmap (bit i of word i/64 set <=> a piece starts at
 * byte i; total/64 + 1 words, the bit at `total` is a sentinel) for the batch.  Host buffers. */
tkz_status tkz_pretokenize_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets,
                                int64_t n_docs, uint64_t* out_bitmap_words);
/* BytePairEncode + whole-piece lookup only: piece p = bytes[piece_offsets[p] .. piece_offsets[p+1])
 * is encoded as ONE regex match (arbitrary bytes allowed).  Host buffers. */
tkz_status tkz_encode_pieces(tkz_encoder* e, const uint8_t* bytes, const int64_t* piece_offsets,
                             int64_t n_pieces, int32_t* out_ids, int64_t out_cap,
                             int64_t* out_offsets, int64_t* needed);

/* Options.  TKZ_OPT_PRETOK_SEQUENTIAL: 1 = split with the one-lane-per-document scanner instead of
 * the position-parallel one; both must give identical bitmaps. */
enum { TKZ_OPT_PRETOK_SEQUENTIAL = 1,
       /* The piece memo: the device form of the reference's LRUCache (LRUCache.cs, used at TikTokenizer.cs:254,270): pieces of up to 16
        * bytes that had to be merged leave their (up to 4) tokens in a 524,288-slot (16 MB) table on the device and later batches take them from
        * there instead of running BytePairEncode again.  A pure memo: ids are identical with and without it.  Value 0 = off, 1 = on
        * (default), 2 = on and emptied.  Set options while no call of the encoder is in flight (2 is refused with TKZ_E_ARG otherwise). */
       TKZ_OPT_PIECE_MEMO = 2,
       /* 1: the batch path counts what it meets (tkz_encoder_piece_stats); 0 (default): it does not -- the counting adds a few atomics per
        * wavefront and one small kernel per batch, so measure with it off. */
       TKZ_OPT_PIECE_STATS = 3,
       /* Promoted pieces.  The memo's answers never change, so the encoder moves its hottest entries into the whole-piece key tables themselves: such
        * a piece is then found by the lookup every piece goes through anyway (TikTokenizer.cs:262 -- with its <= 4 tokens in place of a rank) instead of
        * being listed, looked up in the memo and answered again in every batch.  Same ids by construction.  Value 1 (default): automatic -- the first
        * batch of at least 8 MB on the batch path counts the memo's hits per slot and the hottest entries (at most 65,536) are promoted when it ends (the
        * memo is copied back and the key tables rebuilt on the host: tens of milliseconds, once), once more a gigabyte of text later, and again whenever
        * the text has drifted (TKZ_OPT_ADAPT); 0: never automatically; 2: promote now whatever the memo holds; 3: drop every promotion.  2 and 3 are refused
        * with TKZ_E_ARG while a call is in flight. */
       TKZ_OPT_PROMOTE = 4,
       /* tuning knobs of the automatic promotion: the smallest batch (bytes) that may be a learning batch (default 8 MB), and the most promoted
        * pieces the key tables hold (default 65,536; at most 2^22) */
       TKZ_OPT_PROMOTE_MIN_BYTES = 5, TKZ_OPT_PROMOTE_CAP = 6,
       /* cl100k's `(?i:'s|'t|'re|'ve|'m|'ll|'d)` as the host's engine reads it: 0 (default) = ASCII case pairs only -- net6.0, the reference's target; 1 =
        * with .NET >= 7's case-equivalence tables, under which U+017F (long s) is an `s`: an apostrophe at which a match starts, followed by U+017F,
        * is the contraction (none of the other letters of the seven literals has a non-ASCII equivalent).  No effect on the other patterns (pattern 1 is
        * case-sensitive, o200k lists its case variants). */
       TKZ_OPT_CASE_EQUIVALENCE = 7,
       /* Batches of at most this many bytes are run for latency rather than throughput (default 16 MB; 0: never): at these sizes the call waits for the
        * slowest wavefront of each kernel, so the merge of the long missed pieces is dealt out in units of 4 sub-tiles instead of 64 (93 -> 44 us of a 1 MB
        * call) and its queue of very long pieces gets a full grid.  Same ids either way.  (TKZ_LATENCY_BYTES in the environment sets the value an encoder
        * is created with.) */
       TKZ_OPT_LATENCY_BYTES = 8,
       /* The cache adapts (default 1).  The reference's LRUCache evicts and refills for ever (LRUCache.cs:79-121); the device memo takes no entry once it is
        * full and a promoted piece stays promoted.  With this option on the encoder follows, from batch to batch, the share of pieces that miss its key
        * tables as a whole (counted by a kernel that runs anyway); when that share has left the level at which it settled after the last promotion -- by
        * more than a quarter and a percentage point, either way, 256 MB of text or more after it -- the encoder learns again: every promotion is dropped
        * (so a piece that stopped hitting is not chosen again), the memo is emptied (while no other call is in flight: a host call that is cut into chunks does so at its first chunk, before the second is
        * begun, so the window may wait for the next call), the next learning window counts
        * hits and the hottest pieces of the text as it is now are promoted.  Also with it on: the learning rounds go on (1, 2, 4, 8 ... GB apart: a change
        * of text that does not move the miss share is still learnt; a round only adds pieces; a list that later rounds have filled to nine tenths of its cap starts over, one that a single window filled stays
        * until the text drifts), and batches smaller
        * than TKZ_OPT_PROMOTE_MIN_BYTES add up to a learning window instead of never learning.  0: learn in the first batch of at least that size and once more a gigabyte later, never again
        * (round 5's behaviour).  Same ids either way. */
       TKZ_OPT_ADAPT = 9 };
tkz_status tkz_encoder_set_option(tkz_encoder* e, int32_t option, int64_t value);

/* ---- measurement ------------------------------------------------------------------------- */

enum { TKZ_K_DOCMARK = 0, TKZ_K_PRETOK = 1, TKZ_K_PROBE = 2 /* k_probe alone */, TKZ_K_SCAN = 3, TKZ_K_PLACE = 4,
       TKZ_K_DOCOFFS = 5, TKZ_K_MERGE_LONG = 6 /* k_giant_order + k_giant_merge + k_long_count / scan / k_long_scatter + k_merge_long_q + k_merge_coop */, TKZ_K_MERGE_SHORT = 7 /* k_merge_short alone */,
       TKZ_K_COUNT = 8 };
/* When enabled, every kernel launch of tkz_encode_batch_device is bracketed by HIP events on the
 * launch stream; tkz_encoder_kernel_ms returns the accumulated milliseconds and launch counts per
 * kernel since the last reset (arrays of TKZ_K_COUNT).  Not inside any bracket (microseconds each): the fill of the workspace's zero region,
 * k_doccount2 and the scan of its counts, k_list_stats (which also finds the giant pieces and fills k_merge_coop's queue); of a trim call
 * (tkz_encode_batch_trim_device) k_trim_cut, the scan of the kept lengths and k_trim_gather, which run behind TKZ_K_DOCOFFS.
 * Of a span call (tkz_encode_batch_spans_device) the TKZ_K_DOCOFFS bracket holds k_docoffs over the pieces AND the span stage behind it (the fill of the interior
 * bitmap, k_tokspan_mark, k_tokspan_count, two scans, k_tokspan_write): the closing event is recorded again behind the stage.  Of a chunk call
 * (tkz_encode_batch_chunks_device) likewise: k_docoffs over the pieces and the chunk stage (the two walks, their scan, the unit counts, k_chunk_units).
 * Of a packed call (tkz_encode_batch_packed_device) the TKZ_K_DOCOFFS bracket holds k_docoffs over the documents and the packing stage behind it
 * (k_pack_count, the scan of its counts, k_pack_write), closed again behind the stage in the same way.  Of a padded call (tkz_encode_batch_padded_device)
 * likewise: k_docoffs over the documents, k_pad_lens and k_pad_write; of a bucketed call (tkz_encode_batch_bucketed_device): k_docoffs, k_pad_lens, the sort's
 * passes, k_bkt_table, its scan and k_bkt_write; of a budgeted call (tkz_encode_batch_budgeted_device): k_docoffs, k_pad_lens, the sort's passes, k_tbk_mark
 * twice with its scan, k_tbk_chain, the scan of the runs' buckets, k_tbk_table, its scan and k_tbk_write; of a pair call (tkz_encode_batch_pairs_device):
 * k_docoffs over the documents, k_pair_lens and k_pair_write.
 * A batch that runs the long pieces' kernels beside k_merge_short (tkz_encoder_side_by_side_batches) has k_merge_long_q and k_merge_coop INSIDE the
 * TKZ_K_MERGE_SHORT bracket -- the three side by side, from the fork to the join -- and only what runs in front of them (the giant pieces, the class
 * queue's counting, scan and scatter) in TKZ_K_MERGE_LONG.  A batch of at most TKZ_OPT_LATENCY_BYTES likewise: its TKZ_K_MERGE_SHORT bracket is k_merge_latency
 * (k_merge_short's workgroups and tkz_merge_long_chunks in one launch) + k_merge_coop, its TKZ_K_MERGE_LONG bracket the giant pieces' two kernels. */
tkz_status tkz_encoder_set_profiling(tkz_encoder* e, int32_t enabled);
tkz_status tkz_encoder_kernel_ms(tkz_encoder* e, double* ms, int64_t* launches, int32_t reset);
/* o200k only, informational: of the 4 KiB blocks of the last batch, how many the ASCII block scanner handed on (blocks with multi-byte
 * chars or a state it cannot carry), and how many of those the multi-byte block scanner handed on to the sequential matcher. */
void tkz_encoder_pretok_leftovers(const tkz_encoder* e, int64_t* after_ascii_scanner, int64_t* after_multibyte_scanner);
/* The single-launch path: a host-buffer call (tkz_encode_utf8 / _utf16, tkz_encode_batch_utf8) whose batch is at most 128 KiB in at most
 * 8192 documents (o200k: at most 64 KiB, documents of at most 1 KiB) runs as ONE kernel launch that reads the text from, and writes the ids into, page-locked host memory
 * (no copy commands; 16 launches otherwise).  Informational: how many calls took it, and how many of those the kernel handed back to the
 * batch path (a piece of more than 1024 bytes or one of more than 256 that is not a key, an error to diagnose, workspace to grow). */
void tkz_encoder_small_path_calls(const tkz_encoder* e, int64_t* calls, int64_t* handed_back);
/* development: the shader-clock stamps the last single-launch kernel left at the end of each of its phases (16 values; returns how many) */
int32_t tkz_encoder_small_path_phases(const tkz_encoder* e, int64_t* clocks16);
/* What the batches since the last reset met, with TKZ_OPT_PIECE_STATS on (8 values): [0] batches, [1] pieces (regex matches), [2] pieces of
 * at most 16 bytes that missed the vocabulary as a whole (TikTokenizer.cs:262 -> :268), [3] of 17..1024 bytes (merged a lane each up to 128 bytes, a wavefront each beyond), [4] of more than 1024 bytes (a workgroup each),
 * [5] piece-memo lookups and [6] hits among them (the misses went through BytePairEncode), [7] promoted pieces the key tables hold now
 * (TKZ_OPT_PROMOTE: they count as whole-piece hits).  Whole-piece hit rate =
 * 1 - ([2] + [3] + [4]) / [1]. */
tkz_status tkz_encoder_piece_stats(tkz_encoder* e, int64_t* out8, int32_t reset);
/* TKZ_OPT_ADAPT, informational (8 values; waits for a promotion being built in the background): [0] promotions installed so far, [1] times the encoder
 * decided to learn again, [2] promoted pieces the key tables hold now, [3] replaced table images not freed yet (they go when no call is in flight),
 * [4] the share of pieces that missed the key tables as it settled after the last promotion, in millionths (-1: not settled yet), [5] the same share
 * over the recent batches (-1: none yet), [6] bytes encoded since the key tables last changed, [7] bytes of the learning window in progress. */
tkz_status tkz_encoder_adapt_stats(tkz_encoder* e, int64_t* out8);
/* Slots of the piece memo (TKZ_OPT_PIECE_MEMO) and slots per bucket, informational; the bucket a piece of 1..16 bytes would use
 * (-1: none -- a piece that holds a zero byte never uses the memo).  The tests use the last one to build pieces that contend for one bucket. */
int64_t tkz_encoder_memo_slots(const tkz_encoder* e);
int32_t tkz_encoder_memo_ways(const tkz_encoder* e);
int64_t tkz_encoder_memo_bucket(const tkz_encoder* e, const uint8_t* piece, int32_t len);
/* Allocates, now, the workspace of a batch of up to max_bytes bytes in up to max_docs documents (about 7.8 device bytes per input byte: records, miss
 * lists, bitmaps, scratch, the staging of the host-buffer entry points, streams): replaces the allocations the first batch call of a fresh encoder
 * otherwise makes inside the call.  The reference pays its construction costs in TokenizerBuilder.CreateTokenizer (TokenizerBuilder.cs:210-213) --
 * call this right after tkz_encoder_create.  Batches up to that size then allocate nothing; larger ones grow the workspace as before.  An encoder whose
 * host threads run batches concurrently reserves one workspace per call of this function. */
tkz_status tkz_encoder_reserve(tkz_encoder* e, int64_t max_bytes, int64_t max_docs);
/* Device bytes currently held by the encoder (tables + workspace). */
int64_t tkz_encoder_workspace_bytes(const tkz_encoder* e);
/* Informational: batches whose kernels of the long missed pieces (k_merge_long_q, k_merge_coop) ran BESIDE k_merge_short on streams of their own instead of behind it --
 * a batch above TKZ_OPT_LATENCY_BYTES on a workspace whose previous such batch left at most 2^20 long misses (the launch sequence of a large batch). */
int64_t tkz_encoder_side_by_side_batches(const tkz_encoder* e);
/* Informational: copies of results (ids, offsets) of host-buffer calls that left the device on a copy engine of their own, named through the HSA runtime
 * (csrc/tkz_sdma.h) -- the chunks of a batch of 12 MB or more whose result buffers are page-locked (tkz_host_alloc, hipHostMalloc).  0 when the runtime
 * library or its entry points are missing, or TKZ_D2H_ENGINE=-1: such downloads go through hipMemcpyAsync. */
int64_t tkz_encoder_engine_downloads(const tkz_encoder* e);
const char* tkz_kernel_name(int32_t k);

/* Synthetic corpus of BASELINE.json's configs, generated ON DEVICE by a counter-based generator
 * (csrc/tkz_corpus.h); the same function compiled for the host regenerates any document for spot
 * checks.  kind: 1 = ASCII English/code-like (configs 1,2,4), 2 = mixed UTF-8 CJK+emoji (config 3),
 * 3 = long-context with long single-class runs (config 5), 5 = words of the 4096-word table drawn uniformly, each behind a single space
 * (back to back and taken as ONE document this is the shape of the reference's own benchmark, PerfBenchmark/Program.cs:14-32).
 * d_doc_offsets (n_docs+1 entries, device) is always written; d_bytes (device, capacity cap_bytes) is
 * filled when non-NULL and large enough; *total_bytes is returned either way, so a first call with
 * d_bytes == NULL sizes the buffer.  Document d depends only on (kind, seed, first_doc + d, min_len, max_len). */
tkz_status tkz_corpus_generate_device(int32_t device, int32_t kind, uint64_t seed, int64_t first_doc,
                                      int64_t n_docs, int32_t min_len, int32_t max_len,
                                      int64_t* d_doc_offsets, uint8_t* d_bytes, int64_t cap_bytes,
                                      void* hip_stream, int64_t* total_bytes);
/* Host regeneration of ONE document (returns its byte length); buf may be NULL to query the length. */
int64_t tkz_corpus_generate_doc_host(int32_t kind, uint64_t seed, int64_t doc_index, int32_t min_len,
                                     int32_t max_len, uint8_t* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* TKZ_H */
