// tkz_kernels.h -- host-callable launchers of the HIP kernels (tkz_kernels.hip) and the parameter
// blocks they take.
#pragma once
#include <stdint.h>

#include "tkz_simt.h"
#include "tkz_tables.h"

namespace tkz {

constexpr int kThreads = 256;       // workgroup size of every kernel (4 wavefronts)
constexpr int kSub = 1024;          // bytes of corpus per wavefront of k_probe / k_place (a "sub-tile")
constexpr int kHalo = 64;           // bytes staged past the sub-tile (a short piece may straddle the edge)
constexpr int kShortMax = 16;       // pieces up to this many bytes are merged one per lane, 64 to a wavefront, by k_merge_short
#ifndef TKZ_MERGE_GROUP
#define TKZ_MERGE_GROUP 16
#endif
constexpr int kMergeGroup = TKZ_MERGE_GROUP;   // sub-tiles per wavefront of k_merge_short ("group")
constexpr int kDenseCap = 256 * kMergeGroup;   // tokens of merged short pieces a group keeps packed (what does not fit waits in tmp, like the long pieces' tokens)
#ifndef TKZ_ARENA_DWORDS
#define TKZ_ARENA_DWORDS 2560
#endif
constexpr int kArenaDwords = TKZ_ARENA_DWORDS;  // LDS arena of k_merge_long: a long miss of a batch gets its bytes + 1 dword + 1 bit per byte out of it (2 dwords per byte for
                                    // vocabularies with ranks of 2^21 and more, which keep an ids[] array: tkz_bpe.h)
constexpr int kArenaPiece = 1024;   // ... so pieces up to this many bytes are merged one per lane there (256 + tkz_bpe_var_dwords(1024) = 2336 <= kArenaDwords)
#ifndef TKZ_LANE_PIECE
#define TKZ_LANE_PIECE 128
#endif
constexpr int kLanePiece = TKZ_LANE_PIECE;
constexpr int kLongLogDwords = 12, kLongLogMaxLen = 28;      // (28 = TKZ_MID_KEY_MAX: what the MID key table can hold)
constexpr int kSmallLanePiece = 256;  // ... the single-launch kernel (no k_merge_coop there) merges pieces of up to this many bytes a lane each and hands a batch with a longer missed piece back    // ... but a missed piece longer than this is merged by a whole wavefront (k_merge_coop): one lane takes ~n^2 steps, and the kernel waits for it
constexpr int kMaxPiece = 1 << 30;  // longer single pieces are refused (kErrTooLong)
constexpr int kRowsPerWave = 62;    // k_pretok_rows: output rows per wavefront (64 staged rows, one per lane; the outer two are context)
constexpr int kScanBlock = 1024;    // tiles per workgroup in the tile-count scan
constexpr int kRecordLine = 16;     // piece records per 64-byte line: every sub-tile's records start on a line of their own
constexpr int kMissCapMin = 64, kMissCapMax = 1024;   // entries of a sub-tile's miss list: what a workspace starts with, and the most a sub-tile can need (a miss per byte)

enum { K_DOCMARK = 0, K_PRETOK = 1, K_ENCODE = 2, K_SCAN = 3, K_GATHER = 4, K_DOCOFFS = 5, K_HEAVY = 6, K_MERGE_SHORT = 7, K_COUNT = 8 };

#ifdef TKZ_DEVPROF
#define TKZ_DEV_FLAG(P, bit) (((P).ablate & (bit)) != 0)
#else
#define TKZ_DEV_FLAG(P, bit) false
#endif

struct EncodeParams {
    const uint8_t* bytes; int64_t total;
    const uint64_t* startbits; const uint64_t* docbits; int64_t nwords;   // 1 bit / byte, nwords = total/64 + 1
    const int64_t* offs; int64_t n_docs;                                  // n_docs + 1 document offsets
    int32_t* tmp;                 // [total + pad] tokens of a LONG missed piece wait at the piece's own byte position (tokens <= bytes)
    int32_t* dense;               // [groups x kDenseCap] tokens of the short missed pieces of a group of sub-tiles, packed in piece order
    int32_t* tile_count;          // tokens produced by each sub-tile
    int32_t* prank; int64_t prank_cap;   // one record per piece, in piece order (tkz_kernels.hip, "the encode stage")
    const int32_t* pcount;        // pieces that start in each sub-tile
    const int64_t* pbase;         // ... and the exclusive scan of the counts rounded up to 16: where the sub-tile's records (whole lines) start
    uint32_t* mlist; int32_t mcap;       // per sub-tile mcap entries: the short misses from the front, the long ones from the back; answered in place
    uint4* mquad;                 // 16 bytes beside every list entry: a short miss's bytes on the way in, its <= 4 tokens on the way out
    uint32_t* mcount;             // per sub-tile: short misses | long misses << 16
    const int64_t* docord_base;   // per sub-tile: number of distinct document-start positions before it
    int32_t* doc_tok;             // per document-start position (by ordinal): token index inside its sub-tile
    int32_t* counters;            // [0] error bits, [1] the longest miss list seen (kErrMissCap), [2] the longest list above kMissCapMin that fitted (grown lists only),
                                  // [3] sub-tiles with more than 64 list entries ([2], [3]: k_list_stats, grown lists only)
    int32_t latency;              // a batch run for latency (TKZ_OPT_LATENCY_BYTES): the launchers pick the forms with the smaller units of work
    int32_t lane_piece;           // long misses of up to this many bytes are merged a lane each (k_merge_long), longer ones a wavefront each (k_merge_coop): kLanePiece
    uint8_t* heavy_flag; int64_t nsub;                                    // one byte per sub-tile, set by k_probe: bit 0 = long misses in its list, bit 1 = a giant piece, bit 2 = a long miss of more than kLanePiece bytes (k_merge_coop)
                                                                          // (a flag, not a queue: a queue's one counter serialises a million atomics on mixed text)
    int32_t* pool; unsigned long long* pool_head; int64_t pool_cap;       // scratch for pieces > kArenaPiece (int32 units)
    // pieces > kArenaPiece bytes ("giant"): found by k_giant_find, merged by k_giant_merge (one 1024-thread workgroup each); their
    // tokens wait in tmp at the piece's own byte position, their count in giant_cnt[sub-tile of the piece start]
    int64_t* giant_q; unsigned long long* giant_count; int64_t giant_cap; int32_t* giant_cnt;
    unsigned long long* giant_ticket;       // k_giant_merge: next entry of the (longest first) order, giant_q[2 * giant_cap + t], to be taken
    // long misses of more than kLanePiece bytes (k_merge_coop: a wavefront each): queued by k_list_stats as sub-tile << 10 | index in the sub-tile's long list
    uint64_t* coop_q; unsigned long long* coop_count; unsigned long long* coop_ticket; int64_t coop_cap;
    // the long misses of up to lane_piece bytes, binned by length class across the batch (large batches: k_long_count -> scan -> k_long_scatter -> k_merge_long_q).
    // (a small batch takes them in the chunk form instead: k_merge_latency).  lq_cnt / lq_base: [16 classes x chunks of 64 sub-tiles]; lq: sub-tile << 30 | list index << 20 | (len - 1) << 10 | byte in the sub-tile
    int32_t* lq_cnt; int64_t* lq_base; int64_t* lq_total; int64_t* lq_bsum; uint64_t* lq; int64_t lq_cap;
    unsigned long long* miss_sums;   // null, or [2]: k_list_stats adds the batch's short and long misses (the sums of mcount) -- TKZ_OPT_ADAPT follows their share of the pieces
    // development builds only (make DEVPROF=1; env TKZ_DEV_ABLATE bit 4): per-phase clock counters of k_probe.  Compiled out of libtkz.so otherwise.
    unsigned long long* devprof;
    int32_t ablate;
    // TKZ_OPT_PIECE_STATS: null, or the encoder's statistics block -- [0] memo lookups, [1] memo hits, [2] short misses, [3] long misses, [4] pieces
    // (what tkz_encoder_piece_stats reports; the timed runs leave it null)
    unsigned long long* stats;
    // a LEARNING batch (tkz_api.cpp): k_merge_long logs the pieces of 17..28 bytes it merged into at most 4 tokens -- {7 dwords of bytes, len | count << 8,
    // 4 tokens} = kLongLogDwords dwords a record, up to long_log_cap records (the counter runs on) -- so that the host can promote the ones that repeat
    // (the indentation runs of source code: "\n" + 19 spaces is a missed piece of 20 bytes that real text holds by the hundred thousand)
    uint32_t* long_log; unsigned long long* long_log_count; int32_t long_log_cap; int32_t long_log_sparse;
    int32_t* pextra;              // null, or (promoted pieces in the tables) per sub-tile: tokens beyond one per piece that its promoted pieces stand for (k_probe -> k_merge_short's counts)
    const uint4* promo;           // token quads of the promoted pieces (TkzTables::promo of the tables this batch was probed with), or null: k_place
    int32_t tc_atomic;            // k_probe zeroes tile_count and k_merge_short ADDS its counts (atomics) instead of storing them: the long-piece kernels, which add theirs, may run beside it (Launch::side)
    int32_t place128;             // launch k_place<128> (two kept list entries per lane) instead of k_place<64>: the previous batch of the workspace was miss-heavy
    // the special entries only (null on the plain path, which then launches the k_probe it always did): bit i set <=> a TAKEN special-token literal starts at
    // byte i -- that piece's record is the literal's id (k_probe_special) --, and the literal table the id is read from (TkzLitTable)
    const uint64_t* specbits; const uint32_t* lit_meta; const uint8_t* lit_blob; int32_t n_lit;
    const uint64_t* lit_repl;     // null, or the replaced-byte bitmap of a UTF-16 special call (launch_lit_scan): k_probe_special names the literal k_lit_scan matched
};

// ---- special tokens on the device (EncodeInternal / FindNextSpecialToken, TikTokenizer.cs:141-170,230-241) ----
// The registered literals in registration order (= the reference's alternation order).  meta: [0..7] the first bytes of all literals as a 256-bit set,
// [8..15] the literals that hold U+FFFD (EF BF BD) as a 256-bit set over their indices, then two dwords per literal: offset into blob | length << 16, id.
constexpr int kLitMax = 256, kLitMaxLen = 128, kLitFffdHead = 8, kLitMetaHead = 16;
struct TkzLitTable { const uint32_t* meta; const uint8_t* blob; int32_t n; int32_t blob_bytes; };
struct TkzLitAllowed { uint64_t m[kLitMax / 64]; };       // bit i: literal i is allowed in this call

// k_small: one launch for a small batch (tkz_kernels.hip).  Input and output live in page-locked host memory the device reads and writes directly.
// (k_small's static LDS: 83.5 KB of gfx950's 160 KB per workgroup -- more than the 64 KB of earlier CDNA parts: the host takes the single-launch path only
//  on a device whose sharedMemPerBlock covers it, the batch path otherwise)
constexpr int kSmallLdsBytesNeeded = 86 * 1024;
constexpr int kSmallMaxBytes = 131072, kSmallMaxBytesO200k = 65536, kSmallMaxDocs = 8192, kSmallMaxDoc = 1024;
// the trim form (tkz_encode_trim_utf8 / _utf16) takes the launch up to this many bytes: the route it replaces -- the batch trim path, the whole chip -- costs
// about the same at every size up to 128 KiB, one workgroup grows with the text.  Scanned on plain text with the launch taken at every size
// (profiles/small_trim/README.md, crossover.jsonl): a/b 0.52 .. 0.66 at 48 KiB, 0.78 .. 0.96 at 96 KiB -- the largest scanned size with the launch ahead in every
// row --, 0.86 .. 1.01 at 104 KiB, 0.92 .. 1.04 at 112, 0.94 .. 1.17 at 128.  A conservative choice, not an interpolated crossover: nothing between 96 and 104 KiB
// was scanned, and the gpt2 rows are still ahead at 112.
// (development: -DTKZ_SMALL_TRIM_MAX_BYTES=131072 builds the library the scan was taken with: the launch at every size the plain entries allow)
#ifndef TKZ_SMALL_TRIM_MAX_BYTES
#define TKZ_SMALL_TRIM_MAX_BYTES 98304
#endif
constexpr int kSmallTrimMaxBytes = TKZ_SMALL_TRIM_MAX_BYTES;
static_assert(kSmallTrimMaxBytes > 0 && kSmallTrimMaxBytes <= kSmallMaxBytes, "the trim form runs inside the single-launch kernel's limits");
struct SmallArgs {
    const uint8_t* h_bytes; const int64_t* h_offs;          // the batch, in page-locked host memory (h_bytes kSmallMaxBytes + 64 long)
    int32_t* out; int64_t out_cap; int64_t* out_offs;       // ids and document offsets, page-locked host memory
    int64_t* h_result;                                      // [0] status (0 done, 1 take the batch path), [1] error bits, [2] token count, [3] literals taken (the special form)
                                                            // [4..19] clock stamps; the trim form: [20] first kept token, [21] kept count, [22] cut_bytes, [23] cut_units
    uint64_t* docbits; uint64_t* startbits;                 // the workspace arrays EncodeParams holds as const, writable
    int32_t* pcount; int64_t* pbase; int64_t* docord_base; int64_t* tile_base;
    int32_t counter_words;                                  // 32-bit words of the counter block to zero
    int64_t* counts3[2];                                    // {n_docs, n_bytes, n_tokens} of the batch, on the device: the encoder's block and the workspace's (either may be null)
    // the special form (k_small<true>; n_taken null: the plain one, which reads none of these): the registered literals, the ones this call allows, the four
    // bitmaps of the literal search (nwords + 8 words each), the counter of the literals taken (inside the counter block: zeroed with it; h_result[3] on
    // return) and -- text transcoded from UTF-16 on the host while a registered literal holds U+FFFD -- the replaced-byte bitmap in page-locked host memory
    // (launch_lit_scan's `repl`; EncodeParams::lit_repl is the same pointer), or null
    TkzLitTable lit; TkzLitAllowed allowed;
    uint64_t* candbits; uint64_t* segbits; uint64_t* specbits; uint64_t* endbits;
    unsigned long long* n_taken;
    const uint64_t* repl;
    // the trim form (k_small<SPECIAL, true>: tkz_encode_trim_utf8 / _utf16, ONE document; trim 0: the other forms, which read none of these): the side
    // (tkz_trim_side) and the maximum.  EncodeParams::docbits is the PIECE-start bitmap then, doc_tok holds an entry per piece, `out` holds the untrimmed ids
    // (out_cap kSmallMaxBytes) and the host copies [h_result[20], + h_result[21]) of them
    int32_t trim; int32_t trim_side; int64_t trim_max;
};

// k_dec_small: one launch for Decode of ONE id list (tkz_kernels.hip).  The ids come from, and the bytes (UTF-8 form) or code units (UTF-16 form) go to,
// page-locked host memory.  The two figures are what the page-locked block holds, not tuned thresholds: a list of more ids takes the batch path, and so does one the
// kernel hands back because it decodes to more bytes.  (Its static LDS: 81 KB, inside what the host already checks for k_small, kSmallLdsBytesNeeded.)
constexpr int kDecSmallMaxIds = 32768, kDecSmallMaxBytes = 131072;
// ... and the route threshold on the id count, measured (profiles/small_decode/README.md): the launch is ahead of the batch path at every size up to the capacity
// (development: -DTKZ_SMALL_DECODE_MAX_IDS=n builds a library that takes the launch up to n ids)
#ifndef TKZ_SMALL_DECODE_MAX_IDS
#define TKZ_SMALL_DECODE_MAX_IDS 32768
#endif
constexpr int kDecSmallRouteIds = TKZ_SMALL_DECODE_MAX_IDS;
static_assert(kDecSmallRouteIds >= 0 && kDecSmallRouteIds <= kDecSmallMaxIds, "the route threshold lies inside the block's capacity");
struct DecSmallArgs {
    const int32_t* h_ids; int64_t n_ids;                    // the id list, page-locked host memory (1 .. kDecSmallMaxIds)
    void* h_out;                                            // page-locked: kDecSmallMaxBytes bytes (UTF-8 form) or as many code units (UTF-16 form)
    int64_t* h_result;                                      // [0] status (0 done, 1 take the batch path: more than kDecSmallMaxBytes bytes), [1] byte total, [2] unit total
                                                            // (UTF-16 form), [4..19] clock stamps
    int32_t utf16;                                          // the output form
    uint8_t* d_bytes; uint64_t* d_docbits;                  // UTF-16 form only, workspace: the decoded bytes (kDecSmallMaxBytes + 64) and their document-start bitmap
                                                            // (kDecSmallMaxBytes / 64 + 1 words: bit 0 and the sentinel at the total)
};

typedef void (*KernelHook)(void* ctx, int kernel_id, int phase /*0 before, 1 after*/, hipStream_t s);
// side / side2 / ev_fork / ev_join / ev_join2: all null, or two more streams and three events of the workspace -- launch_encode runs k_merge_long_q and k_merge_coop there,
// beside k_merge_short on `stream` (a large batch only: EncodeParams::tc_atomic says that the token counts of the sub-tiles are summed with atomics from zero)
struct Launch { hipStream_t stream; KernelHook hook; void* hook_ctx; hipStream_t side = nullptr, side2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr; };

// has_empty: null, or a zeroed word that is set when an item is empty (launch_docoffs)
void launch_docmark(const Launch& L, const int64_t* d_offs, int64_t n_items, int64_t total, uint64_t* bits, int32_t* counters, int32_t* has_empty = nullptr);
// position-parallel Regex.Matches; xq / xcount: queue of row blocks left to the sequential matcher (o200k only)
void launch_pretok_rows(const Launch& L, int pattern, const uint8_t* d_bytes, const int64_t* d_offs, int64_t n_docs, int64_t total,
                        const uint64_t* docbits, uint64_t* startbits, int64_t nrows, const uint8_t* bmp, int32_t* counters,
                        int64_t* xq, unsigned long long* xcount);
void launch_pretok_seq(const Launch& L, int pattern, const uint8_t* d_bytes, const int64_t* d_offs, int64_t n_docs, int64_t total,
                       uint64_t* startbits, const uint8_t* bmp, int32_t* counters);
void launch_ingest(const Launch& L, const uint8_t* h_bytes, int64_t total, uint8_t* d_bytes, const int64_t* h_offs, int64_t n_offs, int64_t* d_offs, void* zero, int64_t zero_bytes);
void launch_probe_sample(const Launch& L, const TkzTables& T, const EncodeParams& P, int64_t nsample);
void launch_encode(const Launch& L, const TkzTables& T, const EncodeParams& P, int64_t nsub);
void launch_small(const Launch& L, const TkzTables& T, const EncodeParams& P, const SmallArgs& A);
void launch_dec_small(const Launch& L, const TkzDecodeTable& D, const DecSmallArgs& A);
// exclusive scan int32 -> int64 (+ grand total); kid = profiling id of the bracket, or -1
// round_to (a power of two): every count is rounded up to a multiple of it before it is summed
void launch_scan(const Launch& L, const int32_t* tile_count, int64_t ntiles, int64_t* bsum, int64_t* tile_base, int64_t* grand, int kid, int round_to = 1);
void launch_place(const Launch& L, const EncodeParams& P, const int64_t* tile_base, int64_t nsub, int32_t* out, int64_t out_cap);
// a count call (tkz_count_*): P.doc_tok as launch_place leaves it and nothing else -- no ids.  dcount: the marks of every sub-tile (launch_doccount2)
void launch_tokcount(const Launch& L, const EncodeParams& P, const int64_t* tile_base, const int32_t* dcount, int64_t nsub);
// (c3a / c3b / c3c: null, or blocks that receive {c3_docs, total, *grand}: launch_counts3's job done by the same launch)
// has_empty: the word launch_docmark set when an item of the batch is empty (zero: the ordinal of item d's mark is d, and the bitmap is not searched)
void launch_docoffs(const Launch& L, const int64_t* d_offs, int64_t n_docs, int64_t total, const int64_t* tile_base,
                    const uint64_t* docbits, const int64_t* docord_base, const int32_t* doc_tok, const int64_t* grand, int64_t* out_offs,
                    const int32_t* has_empty, int64_t c3_docs = 0, int64_t* c3a = nullptr, int64_t* c3b = nullptr, int64_t* c3c = nullptr);
// the counts of two bitmaps per sub-tile in one pass; the scan of one or two count arrays -- a single launch up to 8,192 sub-tiles
void launch_doccount2(const Launch& L, const uint64_t* bits_a, const uint64_t* bits_b, int64_t nwords, int64_t total, int64_t nsub, int32_t* cnt_a, int32_t* cnt_b);
void launch_scan2(const Launch& L, int64_t ntiles, int64_t* bsum, const int32_t* cnt_a, int64_t* base_a, int64_t* grand_a, int round_to_a,
                  const int32_t* cnt_b, int64_t* base_b, int64_t* grand_b, int round_to_b, int kid);
void launch_rebase(const Launch& L, int64_t* offs, int64_t n, int64_t base);
// TKZ_OPT_CASE_EQUIVALENCE: a piece start behind every `'` + U+017F at whose apostrophe a match starts (cl100k on a .NET >= 7 host)
void launch_case_equiv_fix(const Launch& L, const uint8_t* d_bytes, int64_t total, const uint64_t* docbits, uint64_t* startbits);
void launch_miss_stats(const Launch& L, const EncodeParams& P, int64_t nsub);
// the special entries.  launch_lit_scan: candidates (an ALLOWED literal is the first registered literal that matches here and ends inside the document), then the
// literals taken left to right; segbits = docbits | starts | ends of the taken literals, specbits = their starts, endbits = their ends; *n_taken += their number.
// launch_lit_fix (behind the pre-tokenizer, which ran with segbits in the place of docbits): no piece start strictly inside a taken literal.
// launch_seg_offsets: the offsets of the n_seg segments of segbits (n_seg + 1 entries), for the scanners that take offsets (ord_base: the scan of its counts per sub-tile)
// repl: null, or (text transcoded from UTF-16 by launch_u16_write, a registered literal holds U+FFFD) the replaced-byte bitmap, nwords words: bit i set <=> the
// EF BF BD at byte i stands for a lone surrogate.  The reference searches the UTF-16 string, where a lone surrogate is not U+FFFD: a literal that holds U+FFFD
// does not match where its bytes cover such a bit, and the alternation goes on to the next registered literal.
void launch_lit_scan(const Launch& L, const uint8_t* d_bytes, int64_t total, const uint64_t* docbits, int64_t nwords, const TkzLitTable& LT, const TkzLitAllowed& A,
                     uint64_t* candbits, uint64_t* segbits, uint64_t* specbits, uint64_t* endbits, unsigned long long* n_taken, const uint64_t* repl = nullptr);
void launch_lit_fix(const Launch& L, uint64_t* startbits, const uint64_t* segbits, const uint64_t* specbits, const uint64_t* endbits, int64_t nwords);
void launch_seg_offsets(const Launch& L, const uint64_t* segbits, int64_t nwords, int64_t total, int64_t nsub, const int64_t* ord_base, int64_t n_seg, int64_t* seg_offs);
void launch_counts3(const Launch& L, int64_t n_docs, int64_t total, const int64_t* grand, int64_t* out3, int64_t* out3b = nullptr, int64_t* out3c = nullptr);
// UTF-16 documents -> UTF-8 documents (Encoding.UTF8.GetBytes for a batch): lengths + group prefixes, then (after the scan of
// the tile sums) the bytes and the byte offset of every document.  repl: null, or a zeroed bitmap over the OUTPUT bytes (grand / 64 + 1 words) that receives
// one bit at the EF of every U+FFFD written for a lone surrogate (the special entries' literal search: launch_lit_scan)
int64_t u16_tiles(int64_t total_units);
void launch_u16_len(const Launch& L, const uint16_t* units, int64_t total, const uint64_t* docbits, int64_t ntiles, int32_t* grp_prefix, int32_t* tile_sum);
void launch_u16_write(const Launch& L, const uint16_t* units, int64_t total, const uint64_t* docbits, int64_t ntiles, const int64_t* tile_base,
                      uint8_t* out, const int64_t* unit_offs, int64_t n_docs, const int32_t* grp_prefix, const int64_t* grand, int64_t* byte_offs,
                      uint64_t* repl = nullptr);
// piece granularity: byte offset of every piece (n_pieces + 1 entries) and first piece of every document, from the bitmap
void launch_piece_index(const Launch& L, const uint64_t* startbits, int64_t nwords, int64_t total, int64_t nsub, const int64_t* ord_base,
                        int64_t n_pieces, int64_t* piece_offs, const int64_t* d_offs, int64_t n_docs, int64_t* doc_piece);
// EncodeTrimSuffix / EncodeTrimPrefix for a batch (tkz_encode_batch_trim_device): behind the piece-granular launch sequence -- which leaves the untrimmed ids, the
// byte and token offset of every piece and the first piece of every document in the workspace -- the cut of every document (k_trim_cut), the scan of the kept
// lengths into out_offs (n_docs + 1 entries; the kept total also goes to *kept_total) and the kept ids, compacted (k_trim_gather, which also counts cut_units).
// Nothing is written to `out` when the kept total exceeds out_cap.  side: 0 suffix, 1 prefix.  d_max: null (max_tokens holds for all), or a maximum per document
// (a negative one counts as 0).  keep_lo / keep_n / cut_pos: n_docs entries each, workspace; bsum: n_docs / kScanBlock + 2 entries.  cut_bytes / cut_units: the
// caller's, either may be null.  counters: the batch's counter block -- with an error bit set there ([0]) the attempt's offsets mean nothing and nothing is gathered.
struct TrimParams {
    const uint8_t* bytes; const int64_t* offs; int64_t n_docs, total;
    const int64_t* doc_piece; const int64_t* piece_boffs; const int64_t* piece_toffs;
    int32_t side; int64_t max_tokens; const int64_t* d_max;
    int64_t* keep_lo; int64_t* keep_n; int64_t* cut_pos; int64_t* bsum;
    int64_t* cut_bytes; int64_t* cut_units;
    const int32_t* counters;
};
void launch_trim(const Launch& L, const TrimParams& R, const int32_t* ids, int64_t ids_cap, int32_t* out, int64_t out_cap, int64_t* out_offs, int64_t* kept_total);
// Token spans (tkz_encode_batch_spans_device): behind the piece-granular launch sequence with the ids in the caller's buffer -- the interior token starts of the
// pieces of several tokens (k_tokspan_mark, which also writes out_offs, n_docs + 1 entries), the token starts and begun UTF-16 units of every sub-tile, their
// scans, and the document-relative byte and unit position of every token (k_tokspan_write).  intbits: nwords words, zeroed by the caller.  cnt_* / base_*: an
// entry per sub-tile; sums: [2], the scans' totals; bsum: nsub / kScanBlock + 2 entries.  tok_bytes / tok_units: out_cap entries each, either may be null (without
// tok_units the bytes are not read again).  counters: the batch's counter block -- kErrSpanDoc / kErrSpanSum are set there; with an error bit in it, or with
// *grand > out_cap, the span arrays are left alone.
struct SpanParams {
    const uint8_t* bytes; int64_t total; const int64_t* offs; int64_t n_docs;
    const uint64_t* startbits; const uint64_t* docbits; uint64_t* intbits; int64_t nwords, nsub;
    const int64_t* doc_piece; const int64_t* piece_boffs; const int64_t* piece_toffs; int64_t n_pieces;
    const int32_t* ids; int64_t out_cap; const int64_t* grand;
    int32_t* cnt_tok; int32_t* cnt_unit; int64_t* base_tok; int64_t* base_unit; int64_t* sums; int64_t* bsum;
    int64_t* out_offs; int32_t* tok_bytes; int32_t* tok_units; int32_t* counters;
};
void launch_tokspans(const Launch& L, const SpanParams& S, const TkzDecodeTable& D);
// Token-budget chunks (tkz_encode_batch_chunks_device): behind the piece-granular launch sequence with the ids in the caller's buffer -- every document's tokens cut
// into chunks of at most max_tokens that end at item boundaries where one is in reach (tkz.h states the rule).  The documents are walked TWICE: k_chunk_walk counts
// the chunks of every document (doc_cnt, n_docs entries; a document of more than kChunkLongItems items goes on long_list and is counted by a wavefront,
// k_chunk_walk_long), the counts are scanned into doc_chunk_offs (n_docs + 1 entries; the total also goes to *n_chunks), and the same two kernels walk again and
// write chunk_tokens (chunk_cap + 1 entries), chunk_bytes and chunk_units (chunk_cap entries each, either may be null).  The counting walk also writes out_offs
// (n_docs + 1 entries).  The unit starts: the begun units of every span of kChunkUnitSpan bytes of the batch (k_chunk_unitcount -> cnt_unit, nspan entries, scanned
// into base_unit; ubsum: nspan / kScanBlock + 2 entries, usum: the scan's total), then k_chunk_units turns the batch byte positions the writing walk left in chunk_units into units relative to the document.
// long_list: n_docs entries; long_count: one counter, zeroed by the caller; bsum: n_docs / kScanBlock + 2 entries.  counters: the batch's counter block --
// kErrChunkSum is set there; with an error bit in it the counts are 0, and with one, with *grand > out_cap or with *n_chunks > chunk_cap the table is left alone.
constexpr int64_t kChunkLongItems = 1024;
constexpr int kChunkUnitSpan = 128;
struct ChunkParams {
    const uint8_t* bytes; int64_t total; const int64_t* offs; int64_t n_docs;
    const int64_t* doc_piece; const int64_t* piece_boffs; const int64_t* piece_toffs;
    const int32_t* ids; int64_t out_cap; const int64_t* grand; int64_t max_tokens;
    int64_t* doc_cnt; int64_t* bsum; int64_t* long_list; unsigned long long* long_count;
    int64_t nspan; int32_t* cnt_unit; int64_t* base_unit; int64_t* ubsum; int64_t* usum;
    int64_t* out_offs; int64_t* doc_chunk_offs; int64_t* chunk_tokens; int64_t* chunk_bytes; int64_t* chunk_units; int64_t chunk_cap;
    int64_t* n_chunks; int32_t* counters;
};
void launch_chunks(const Launch& L, const ChunkParams& C, const TkzDecodeTable& D);
// Overlapping token-budget chunks (tkz_encode_batch_chunks_overlap_device; tkz.h states the rule): launch_chunks' sequence with walks and a unit kernel of their
// own (k_chunkov_walk, k_chunkov_walk_long, k_chunkov_units; k_chunk_unitcount and the scans are shared).  C is the existing call's block, read as there, except
// that chunk_tokens has chunk_cap entries (no total behind the last chunk).  overlap: 0 <= overlap < C.max_tokens.  chunk_ends: chunk_cap entries, required;
// chunk_end_bytes / chunk_end_units: chunk_cap entries each, either may be null.  The unit stage runs when C.chunk_units or chunk_end_units is given.
struct ChunkOvParams {
    ChunkParams C; int64_t overlap;
    int64_t* chunk_ends; int64_t* chunk_end_bytes; int64_t* chunk_end_units;
};
void launch_chunks_overlap(const Launch& L, const ChunkOvParams& V, const TkzDecodeTable& D);
// Packed rows (tkz_encode_batch_packed_device; tkz.h states the rule): behind the PLAIN document-granular launch sequence.  ids / offs are the unframed ids and
// their n_docs + 1 document offsets as k_place / k_docoffs left them: in the workspace when a bos or eos id frames the documents (every id moves), the caller's
// own out / out_offs when none does (ids == out: no id is moved, offs == out_offs: they stand).  The stream is dealt out in tiles of kPackTile positions, a
// wavefront each: k_pack_count counts the segment starts of every tile of the stream (cnt, ntile entries, ntile = the tiles of total_bytes + f * n_docs
// positions, which the stream cannot exceed), launch_scan turns them into base (bsum: ntile / kScanBlock + 2 entries) and the total, and k_pack_write writes the
// framed ids, pad_id over [T, n_rows * row_len), pos (out_cap entries, may be null), seg_starts (seg_cap + 1 entries, may be null) and the framed out_offs.
// totals: {T, n_rows, n_segs}.  counters: the batch's counter block -- with an error bit in it ([0]) nothing of the caller's is touched; with
// n_rows * row_len > out_cap, or seg_starts given and n_segs > seg_cap, the totals are all that is written.
constexpr int kPackTile = 2048;
constexpr int kPackGridMax = 2048;     // workgroups of the two kernels: they stride over the tiles beyond
struct PackParams {
    const int32_t* ids; int64_t ids_cap; const int64_t* offs; int64_t n_docs; const int64_t* grand;
    int32_t bos_id, eos_id, pad_id; int64_t row_len;
    int32_t* out; int64_t out_cap; int64_t* out_offs; int32_t* pos; int64_t* seg_starts; int64_t seg_cap;
    int32_t* cnt; int64_t ntile; int64_t* base; int64_t* bsum; int64_t* totals;
    const int32_t* counters;
};
void launch_pack(const Launch& L, const PackParams& K);
// Padded rows (tkz_encode_batch_padded_device; tkz.h states the rule): behind the PLAIN document-granular launch sequence, whose uncut ids (ids, ids_cap entries)
// and n_docs + 1 document offsets (offs) stay in the workspace.  k_pad_lens, a lane a document: the kept count and the framing into lens (the caller's, n_docs
// entries: len[d] = k[d] + f), the source index of the first kept id into src (n_docs entries, workspace), offs copied to out_offs (may be null), and the largest
// len and the number of cut documents of every workgroup into part_len / part_cut (kPadGridMax entries each, workspace; nparts of them are written: the grid).
// k_pad_write: every wavefront reduces the partials to the width W and n_cut, one lane stores totals = {*grand, W, n_cut}, and when n_docs * W <= out_cap the
// rows are written by output position in tiles of kPadTile, a wavefront each: out, mask (may be null), pos (may be null), n_docs * W entries each.  It reads
// lens and src only -- not offs, max_len or cut_side --, so a cut of another granularity in front of it can fill the two arrays itself.
// counters: the batch's counter block -- with an error bit in it ([0]) nothing of the caller's is touched and the totals are not written.
constexpr int kPadTile = 1024;
constexpr int kPadGridMax = 2048;      // workgroups of the two kernels: they stride over the documents / tiles beyond
struct PadParams {
    const int32_t* ids; int64_t ids_cap; const int64_t* offs; int64_t n_docs; const int64_t* grand;
    int32_t bos_id, eos_id, pad_id; int64_t max_len; int32_t cut_side, pad_side; int64_t pad_multiple;
    int32_t* out; int64_t out_cap; uint8_t* mask; int32_t* pos; int32_t* lens; int64_t* out_offs;
    int64_t* src; int32_t* part_len; int64_t* part_cut; int32_t nparts; int64_t* totals;
    const int32_t* counters;
};
void launch_pad(const Launch& L, PadParams K);
// Length-bucketed padded rows (tkz_encode_batch_bucketed_device; tkz.h states the rule): the padded call's sequence up to and including k_pad_lens -- UNCHANGED:
// pad.lens, pad.src, pad.part_cut, pad.out_offs --, then the documents sorted by len, a bucket table, and the rows with a width per bucket.
//   The sort: a stable LSD radix sort of (key, document), key = len (ascending) or max_len - len (descending: ties keep ascending document index in both), 8 bits
//   a pass, npass = the bytes max_len occupies (the host knows it without waiting: 512 needs two passes).  A pass is k_bkt_hist (a workgroup per tile of
//   kBktSortTile keys: the tile's count of every digit into hist, DIGIT-MAJOR: hist[digit * ntiles + tile]), the exclusive scan of hist into hist_base
//   (launch_scan2; scan_bsum: its block sums) and k_bkt_scatter (the same tile again: a key goes to hist_base[digit][tile] + its rank among the tile's EARLIER
//   keys of its digit).  The first pass reads its keys from pad.lens, the last one stores the documents into `order` (the caller's) and the inverse into `rank`
//   (the caller's, may be null); between them keys and documents ping-pong through key_a / idx_a and key_b / idx_b.
//   The last pass also stores lens and src of every document at its SORTED row (slen, ssrc: n_docs entries each, workspace), which is what the table and the
//   writer read.  Workspace a document: 4 + 8 bytes twice (key_a, idx_a, key_b, idx_b) and 4 + 8 (slen, ssrc).  A tile: 256 counts of 4 bytes (hist) and 256 bases of 8 (hist_base); LDS a workgroup:
//   16 KB (a count per group of 64 keys and digit) + 2 KB (the tile's bases).
//   k_bkt_table, a lane a bucket of bucket_rows sorted rows: maxlen_b is the len (slen) of the bucket's last (ascending) or first (descending) row, W_b from it as the
//   padded rule makes W, widths[b] = W_b (the caller's), bkt_cnt[b] = R_b * W_b (int64, workspace).  The 64-bit scan kernels (k_scan_partials64, k_scan_top,
//   k_scan_final64) make boffs[0 .. n_buckets] of it (workspace; the last entry is P).
//   k_bkt_write: boffs copied to bucket_offs (the caller's), one lane stores totals = {*grand, P, n_cut} (n_cut from pad.part_cut), and when P <= out_cap the rows
//   by output position in tiles of kBktTile, a wavefront each, grid-strided: one search over boffs a tile, then bucket, row and column carried forward.
// counters: as PadParams -- with an error bit nothing of the caller's is touched.
constexpr int kBktSortTile = 1024;     // keys a workgroup of k_bkt_hist / k_bkt_scatter (kBktSortTile / 64 groups of 64, four a wavefront)
constexpr int kBktTile = 1024;         // output positions a wavefront of k_bkt_write
struct BktParams {
    PadParams pad;
    int64_t bucket_rows, n_buckets; int32_t descending, npass;
    int64_t* order; int64_t* rank; int64_t* bucket_offs; int32_t* widths;
    uint32_t* key_a; int64_t* idx_a; uint32_t* key_b; int64_t* idx_b;
    int32_t* hist; int64_t* hist_base; int64_t* scan_bsum; int64_t* hist_total;
    int64_t* bkt_cnt; int64_t* boffs; int32_t* slen; int64_t* ssrc;
};
int bkt_passes(int64_t max_len);                               // 1 .. 4
int64_t bkt_sort_tiles(int64_t n_docs);
void launch_bucketed(const Launch& L, BktParams K);
// Token-budget buckets (tkz_encode_batch_budgeted_device; tkz.h states the rule): the bucketed call's sequence up to and including the sort's last k_bkt_scatter --
// UNCHANGED: order, rank, slen, ssrc --, then the sorted rows cut greedily into buckets of at most bucket_rows rows and rows * width <= token_budget positions.
// The host never learns n_buckets before the call ends: every grid and scan below is sized from n_docs, bucket_cap and out_cap.
//   Runs.  A run is a maximal stretch of sorted rows of one width w(slen).  k_tbk_mark, a lane a sorted row, a workgroup per tile of kTbkMarkTile rows: pass 0
//   stores the marks (w differs from the row before) of every group of 64 rows into mark_cnt and clears run_nbk; launch_scan2 makes mark_base and *n_runs of
//   them; pass 1 stores (first row, width) of run mark_base[group] + the marks below the lane into run_first / run_w.  run_cap = tbk_run_cap(): the runs a
//   batch can have, min(n_docs, ceil(L / M) + 1), 2 when M == 0.
//   k_tbk_chain, ONE wavefront: the only sequential stage walks the RUNS, not the buckets.  Inside a run every bucket has R_w = min(B, T / w) rows (B when
//   w == 0), so it stores a run that buckets start in the entry row (run_entry), R_w (run_r), the buckets that start in the run and end with R_w rows
//   (run_nreg) and, ascending, the end of the bucket that crosses the run's end (run_cross, 0: none); run_nbk: the buckets that start in the run.  The 64 lanes
//   look at the next kTbkLook runs together: ascending for the last run the crossing bucket reaches, descending for the run the next entry lies in.  It also
//   adds up fig = {n_buckets, P}.  Its steps are bounded by the runs, whatever n_buckets is.
//   launch_scan2 makes run_bbase (the first bucket of every run) of run_nbk.  k_tbk_table, a lane a bucket below tbl_cap = min(n_docs, bucket_cap): its run by
//   one search over run_bbase, then brow[b] (first sorted row), bw[b] (W_b) and bkt.bkt_cnt[b] = R_b * W_b; the 64-bit scan makes bkt.boffs of them.
//   k_tbk_write: one lane stores pad.totals = {*grand, P, n_cut} and *n_buckets_out; with n_buckets <= bucket_cap the three bucket arrays are copied to the
//   caller's (bkt.bucket_offs, bucket_rows_out, bkt.widths); with P <= out_cap as well the rows are written as k_bkt_write writes them, a bucket's first row and
//   row count read from brow.
// Workspace beside the sort's: 4 bytes a group of 64 rows twice (mark_cnt, mark_base: 12), 56 bytes a run, 28 bytes a bucket below tbl_cap, 16 bytes of figures.
constexpr int kTbkMarkTile = 256;      // sorted rows a workgroup of k_tbk_mark (a count per group of 64)
constexpr int kTbkLook = 64;           // runs the chain looks at together: a lane each
struct TbkParams {
    BktParams bkt;
    int64_t token_budget, bucket_cap, tbl_cap, run_cap;
    int64_t* bucket_rows_out; int64_t* n_buckets_out;
    int32_t* mark_cnt; int64_t* mark_base; int64_t* n_runs;
    int64_t* run_first; int32_t* run_w; int64_t* run_entry; int64_t* run_r; int64_t* run_nreg; int64_t* run_cross; int32_t* run_nbk; int64_t* run_bbase;
    int64_t* fig; int64_t* brow; int32_t* bw;
};
int64_t tbk_run_cap(int64_t n_docs, int64_t max_len, int64_t pad_multiple);
int64_t tbk_mark_groups(int64_t n_docs);
void launch_budgeted(const Launch& L, TbkParams K);
// Pair rows (tkz_encode_batch_pairs_device; tkz.h states the rule): behind the PLAIN document-granular launch sequence, whose uncut ids (ids, ids_cap entries) and
// n_docs + 1 = 2 * n_pairs + 1 document offsets (offs) stay in the workspace.  k_pair_lens, a lane a pair: the kept counts ka, kb of the two texts by the closed
// forms of the strategy, lens (the caller's, n_pairs entries: ka + kb + f), the row's record into rows (workspace, 3 int64 a pair: the source index of the first kept
// id of A, of B, and len | ka << 32), {ka, kb} into kept (the caller's, n_docs entries, may be null), offs copied to out_offs (may be null), and the largest len and
// the number of cut pairs of every workgroup into part_len / part_cut (kPairGridMax entries each, workspace; nparts of them are written: the grid).
// k_pair_write: every wavefront reduces the partials to the width W and n_cut, one lane stores totals = {*grand, W, n_cut}, and when n_pairs * W <= out_cap the
// rows are written by output position in tiles of kPairTile, a wavefront each: out, mask, type_ids, pos (the last three may be null), n_pairs * W entries each.
// It reads rows only -- not lens, offs, strategy or cut_side.
// counters: the batch's counter block -- with an error bit in it ([0]) nothing of the caller's is touched and the totals are not written.
constexpr int kPairTile = 1024;
constexpr int kPairGridMax = 2048;     // workgroups of the two kernels: they stride over the pairs / tiles beyond
struct PairParams {
    const int32_t* ids; int64_t ids_cap; const int64_t* offs; int64_t n_pairs; const int64_t* grand;
    int32_t bos_id, sep_id, sep_count, eos_id, pad_id; int64_t max_len; int32_t strategy, cut_side, pad_side; int64_t pad_multiple;
    int32_t* out; int64_t out_cap; uint8_t* mask; uint8_t* type_ids; int32_t* pos; int32_t* lens; int32_t* kept; int64_t* out_offs;
    int64_t* rows; int32_t* part_len; int64_t* part_cut; int32_t nparts; int64_t* totals;
    const int32_t* counters;
};
void launch_pairs(const Launch& L, PairParams K);
// batch Decode
int64_t dec_tiles(int64_t total_ids);
void launch_dec_len(const Launch& L, const TkzDecodeTable& D, const int32_t* ids, int64_t total, int64_t ntiles, int32_t* grp_prefix, int32_t* tile_sum);
void launch_dec_write(const Launch& L, const TkzDecodeTable& D, const int32_t* ids, int64_t total, int64_t ntiles, const int64_t* tile_base, uint8_t* out,
                      int64_t out_cap, const int64_t* id_offs, int64_t n_docs, const int32_t* grp_prefix, const int64_t* grand, int64_t* byte_offs, int32_t* counters);
// decoded UTF-8 documents -> UTF-16 documents (Encoding.UTF8.GetString for a batch: every maximal subpart of an ill-formed sequence one U+FFFD): unit counts +
// group prefixes, then (after the scan of the tile sums) the units and the unit offset of every document.  docbits: the document-start bitmap over the bytes
// (launch_docmark over byte_offs), nwords words.  A tile whose units end beyond out_cap is not written.
int64_t u8_tiles(int64_t total_bytes);
void launch_u8_len(const Launch& L, const uint8_t* bytes, int64_t total, const uint64_t* docbits, int64_t nwords, int64_t ntiles, int32_t* grp_prefix, int32_t* tile_sum);
void launch_u8_write(const Launch& L, const uint8_t* bytes, int64_t total, const uint64_t* docbits, int64_t nwords, int64_t ntiles, const int64_t* tile_base,
                     uint16_t* out, int64_t out_cap, const int64_t* byte_offs, int64_t n_docs, const int32_t* grp_prefix, const int64_t* grand, int64_t* unit_offs);
void launch_corpus(hipStream_t s, int kind, uint64_t seed, int64_t first_doc, int64_t n_docs, int min_len, int max_len,
                   int64_t* d_offs, uint8_t* d_bytes, int64_t cap_bytes, int64_t* d_total);

}  // namespace tkz
