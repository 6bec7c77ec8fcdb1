// tkz_api.cpp -- the C ABI of libtkz (include/tkz.h): vocabulary objects, device table upload,
// workspace management and the launch sequence of one encode batch.  HIP only: there is no CPU path.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/tkz.h"
#include "tkz_adapt.h"
#include "tkz_bpe.h"
#include "tkz_corpus.h"
#include "tkz_kernels.h"
#include "tkz_pretok.h"
#include "tkz_promo_select.h"
#include "tkz_sdma.h"
#include "tkz_vocab.h"

namespace {

thread_local std::string g_err;

tkz_status fail(tkz_status s, const std::string& msg) { g_err = msg; return s; }

// The caller's current HIP device is left as it was found: every entry point that needs the encoder's device switches to it
// for the duration of the call only (a host may drive several GPUs, or run torch with another current device).
struct DeviceScope {
    int prev = -1;
    hipError_t enter(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur == dev) return hipSuccess;
        const hipError_t r = hipSetDevice(dev);
        if (r == hipSuccess) prev = cur;
        return r;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(TKZ_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define TKZ_TRY(expr)                                                                                   \
    do {                                                                                                \
        const tkz_status s_ = (expr);                                                                   \
        if (s_ != TKZ_OK) return s_;                                                                    \
    } while (0)

// a grow-only device buffer
// TKZ_LOG_SLOW_MS=<n> in the environment: a batch call that takes longer than n ms on the host says so on stderr, with the time it spent in
// hipMalloc/hipFree (a fresh encoder's first large batch sizes its workspace: gigabytes from the driver, which on some boxes takes seconds)
thread_local int64_t g_alloc_ns = 0;
thread_local int g_alloc_calls = 0;
struct AllocClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~AllocClock() { g_alloc_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); ++g_alloc_calls; }
};
struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    hipError_t ensure(size_t n, int64_t* accounted) {
        if (n <= cap) return hipSuccess;
        AllocClock clock;
        size_t want = std::max(n, cap + cap / 2);
        want = (want + 255) & ~size_t(255);
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, want);
        if (e != hipSuccess && want > n) { want = (n + 255) & ~size_t(255); e = hipMalloc(&q, want); }
        if (e != hipSuccess) return e;
        if (p) (void)hipFree(p);
        if (getenv("TKZ_LOG_ALLOC")) fprintf(stderr, "tkz alloc: %zu -> %zu bytes (asked %zu)\n", cap, want, n);
        *accounted += (int64_t)want - (int64_t)cap;
        p = q; cap = want;
        return hipSuccess;
    }
    void release() { if (p) { AllocClock clock; (void)hipFree(p); } p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// a part of another buffer (not owned)
struct DevView {
    void* p = nullptr;
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct CounterBlock {          // mirrors the device block
    int32_t err; int32_t mneed /* longest miss list of a sub-tile (kErrMissCap) */; int32_t mhigh /* longest list above kMissCapMin that fitted */;
    int32_t over64 /* sub-tiles with more than 64 list entries (k_list_stats; grown lists only) */;
    int64_t grand;
    unsigned long long pool_head;
    int64_t ndocstarts;
    unsigned long long heavy_count;
    int64_t npieces;
    unsigned long long giant_ticket;       // k_giant_merge's work counter
    unsigned long long xcount, xcount2;    // (adjacent: launch_pretok_rows) blocks the o200k ASCII scanner left over, blocks the multi-byte one left over as well
    unsigned long long coop_count, coop_ticket;   // k_list_stats -> k_merge_coop: queued long misses of more than kLanePiece bytes, the next one to be taken
    unsigned long long long_log_count;     // a learning batch: records k_merge_long wanted to log (EncodeParams::long_log)
    int64_t lq_total;                      // long misses in the class queue (the scan of EncodeParams::lq_cnt)
    unsigned long long miss_short, miss_long;   // pieces of the batch that missed the key tables as a whole (k_list_stats: the sums of mcount)
    unsigned long long n_literals;         // the special entries: special-token literals taken (k_lit_resolve)
    int64_t kept_total;                    // the trim entries: ids kept over the whole batch (k_trim_gather)
    int64_t n_chunks;                      // the chunk entries: chunks of the whole batch (k_chunk_walk's writing pass)
    unsigned long long chunk_long;         // ... documents on the wavefront walk's list (k_chunk_walk -> k_chunk_walk_long)
    int64_t pack_total, pack_rows, pack_segs;   // the packed entries: T, n_rows (k_pack_count) and n_segs (the scan of its counts) -- PackParams::totals
    int64_t pad_total, pad_width, pad_cut;      // the padded entries: the uncut total, W and n_cut (k_pad_write) -- PadParams::totals; the bucketed entries: the
                                                // uncut total, P and n_cut (k_bkt_write); the pair entries: the uncut total, W and n_cut (k_pair_write)
    int64_t pad_buckets;                        // the budgeted entries: n_buckets (k_tbk_write), behind their {uncut total, P, n_cut} in the three fields above
    // The LAST field: the fill of a re-run ends in front of it (enqueue_attempt), since k_docmark, which sets it, does not run again then.
    int32_t has_empty, pad_;               // k_docmark -> k_docoffs: a document of the batch is empty (k_docoffs searches the marks' ordinals)
};
constexpr size_t kCountersRerun = offsetof(CounterBlock, has_empty);      // what a re-run clears of the counter block
// ... and the 64-byte block of the length scans (the UTF-16 transcoder, the two decoders): k_docmark's / k_dec_write's error bits, the scans' grand totals
struct LenCounters { int32_t err, pad; int64_t grand /* UTF-8 bytes */, grand16 /* UTF-16 code units (tkz_decode_batch_utf16 only) */; };
const char* const kMsgByteOffsets = "document offsets must start at 0, be non-decreasing and end at the byte count";
const char* const kMsgUnitOffsets = "document offsets must start at 0, be non-decreasing and end at the unit count";
const char* const kMsgIdOffsets = "id offsets must start at 0, be non-decreasing and end at the id count";

void release_each(std::initializer_list<DevBuf*> bufs) { for (DevBuf* b : bufs) b->release(); }

// The buffers of one feature each, with release() directly under the fields: a buffer added to a line is freed by adding it to the line below it.  Workspace
// is made of them (base structs, so a buffer keeps the one name it has everywhere: ws->d_tsum).
struct SpecialBufs {   // the special entries (allocated on their first use): candidates, segment marks (the pre-tokenizer's isolation boundaries), starts and ends of the
    // taken literals; the segments' offsets for the scanners that take offsets
    DevBuf w_candbits, w_segbits, w_specbits, w_endbits, w_segoffs;
    void release() { release_each({&w_candbits, &w_segbits, &w_specbits, &w_endbits, &w_segoffs}); }
};
struct HostStageBufs {   // the host entries' staging: two input sets (chunk k+1 goes up while chunk k is encoded), three output sets; ONE-call entries use set 0
    DevBuf s_bytes[2], s_offs[2], s_out[3], s_outoffs[3];
    void release() { release_each({&s_bytes[0], &s_bytes[1], &s_offs[0], &s_offs[1], &s_out[0], &s_out[1], &s_out[2], &s_outoffs[0], &s_outoffs[1], &s_outoffs[2]}); }
};
struct DecodeBufs {   // Decode: the length scan's buffers (decode_lengths), the host entries' staging of ids, id offsets, bytes and byte (or unit) offsets
    DevBuf d_grp, d_tsum, d_tbase, d_bsum, d_counters, d_ids, d_idoffs, d_out, d_outoffs;
    void release() { release_each({&d_grp, &d_tsum, &d_tbase, &d_bsum, &d_counters, &d_ids, &d_idoffs, &d_out, &d_outoffs}); }
};
struct DecodeUtf16Bufs {   // Decode to UTF-16: the decoded bytes, their document offsets and start bitmap, per-tile / per-group unit counts, the host entry's units
    DevBuf d8_bytes, d8_boffs, d8_docbits, d8_grp, d8_tsum, d8_tbase, d8_bsum, d8_units;
    void release() { release_each({&d8_bytes, &d8_boffs, &d8_docbits, &d8_grp, &d8_tsum, &d8_tbase, &d8_bsum, &d8_units}); }
};
struct DecodeSmallBufs {   // Decode of ONE id list in a single launch (k_dec_small): the page-locked block -- ids | bytes or units | result record --, and for the
    // UTF-16 form the decoded bytes and their start bitmap
    uint8_t* h_dsmall = nullptr; DevBuf ds_bytes, ds_docbits;
    void release() { release_each({&ds_bytes, &ds_docbits}); if (h_dsmall) (void)hipHostFree(h_dsmall); h_dsmall = nullptr; }
};
struct PieceBufs {   // piece-granular entry point: piece byte offsets, token offsets, first piece of every document
    DevBuf p_boffs, p_toffs, p_docp;
    void release() { release_each({&p_boffs, &p_toffs, &p_docp}); }
};
struct TrimBufs {   // the trim entries: the untrimmed ids, {kept token range, cut position} per document and their scan's partial sums; the host entries' maxima and cuts
    DevBuf t_ids, t_keep, t_bsum, t_stage;
    void release() { release_each({&t_ids, &t_keep, &t_bsum, &t_stage}); }
};
struct SpanBufs {   // the span entries: the interior token starts, {token starts, begun units} per sub-tile and their scans (+ the two totals); the host entries' two span arrays
    DevBuf sp_intbits, sp_cnt, sp_base, sp_stage;
    void release() { release_each({&sp_intbits, &sp_cnt, &sp_base, &sp_stage}); }
};
// The UTF-16 batch entry points: code units, their document marks, per-tile / per-group lengths (two sets: the units of chunk k+1 are uploaded and measured while
// chunk k is encoded), the UTF-8 batch they become and its byte offsets (u16_measure / u16_write)
struct U16Stage {
    DevBuf units, offs, docbits, grp, tsum, tbase, bsum, counters, boffs, bytes; LenCounters* h = nullptr;
    DevBuf repl;       // the replaced-byte bitmap of the chunk's UTF-8 bytes (k_u16_write): special calls with a registered literal that holds U+FFFD only
    static size_t repl_bytes(int64_t n_bytes) { return (size_t)(n_bytes / 64 + 8) * 8; }
    hipError_t ensure(int64_t max_units, int64_t max_docs, int64_t* acc, bool with_repl = false) {      // room for a chunk of max_units code units in max_docs documents
        if (with_repl) { const hipError_t r = repl.ensure(repl_bytes(3 * max_units), acc); if (r != hipSuccess) return r; }      // (a unit is at most three bytes)
        const int64_t nw = max_units / 64 + 1, nt = tkz::u16_tiles(max_units), nblk = (nt + tkz::kScanBlock - 1) / tkz::kScanBlock;
        const std::pair<DevBuf*, size_t> want[] = {{&units, (size_t)(max_units + 64) * 2}, {&offs, (size_t)(max_docs + 1) * 8}, {&docbits, (size_t)(nw + 8) * 8},
                                                   {&grp, (size_t)nt * 64 * 4}, {&tsum, (size_t)nt * 4}, {&tbase, (size_t)nt * 8}, {&bsum, (size_t)(nblk + 1) * 8},
                                                   {&counters, 64}, {&boffs, (size_t)(max_docs + 1) * 8}};
        for (const auto& w : want) { const hipError_t r = w.first->ensure(w.second, acc); if (r != hipSuccess) return r; }
        return h ? hipSuccess : hipHostMalloc((void**)&h, 64, 0);
    }
    void release() {
        release_each({&units, &offs, &docbits, &grp, &tsum, &tbase, &bsum, &counters, &boffs, &bytes, &repl});
        if (h) (void)hipHostFree(h);
        h = nullptr;
    }
};
// Encoding.UTF8.GetBytes on the device, in two steps; the caller waits between them in its own way (the chunk pipeline: an event; the trim entry: the null stream).
// On L's stream: the document marks of the units in U.units / U.offs, the UTF-8 length of every unit, their scan; the error bits and the total on their way to U.h.
hipError_t u16_measure(U16Stage& U, const tkz::Launch& L, int64_t n_units, int64_t n_docs) {
    LenCounters* const blk = U.counters.as<LenCounters>();
    const int64_t nt = tkz::u16_tiles(n_units);
    hipError_t r = hipMemsetAsync(U.counters.p, 0, 64, L.stream);
    if (r == hipSuccess) r = hipMemsetAsync(U.docbits.p, 0, (size_t)(n_units / 64 + 1 + 8) * 8, L.stream);
    if (r != hipSuccess) return r;
    launch_docmark(L, U.offs.as<int64_t>(), n_docs, n_units, U.docbits.as<uint64_t>(), &blk->err);
    launch_u16_len(L, U.units.as<uint16_t>(), n_units, U.docbits.as<uint64_t>(), nt, U.grp.as<int32_t>(), U.tsum.as<int32_t>());
    launch_scan(L, U.tsum.as<int32_t>(), nt, U.bsum.as<int64_t>(), U.tbase.as<int64_t>(), &blk->grand, -1);
    return hipMemcpyAsync(U.h, U.counters.p, 16, hipMemcpyDeviceToHost, L.stream);
}
// Once U.h has arrived: bad unit offsets are refused; else U.bytes is sized for the *n_bytes of UTF-8 and these and their offsets (U.boffs) are written on L's stream.
tkz_status u16_write(U16Stage& U, const tkz::Launch& L, int64_t n_units, int64_t n_docs, bool with_repl, int64_t* acc, int64_t* n_bytes) {
    if (U.h->err & kErrOffsets) return fail(TKZ_E_ARG, kMsgUnitOffsets);
    *n_bytes = U.h->grand;
    HIP_TRY(U.bytes.ensure((size_t)*n_bytes + 64, acc));
    if (with_repl) HIP_TRY(hipMemsetAsync(U.repl.p, 0, U16Stage::repl_bytes(*n_bytes), L.stream));
    launch_u16_write(L, U.units.as<uint16_t>(), n_units, U.docbits.as<uint64_t>(), tkz::u16_tiles(n_units), U.tbase.as<int64_t>(), U.bytes.as<uint8_t>(), U.offs.as<int64_t>(), n_docs,
                     U.grp.as<int32_t>(), &U.counters.as<LenCounters>()->grand, U.boffs.as<int64_t>(), with_repl ? U.repl.as<uint64_t>() : nullptr);
    return TKZ_OK;
}

}  // namespace

namespace tkz { tkz_status set_error(tkz_status s, const std::string& msg) { return fail(s, msg); } }   // (tkz_comm.cpp)

struct tkz_vocab { tkz::Vocab v; };

// Everything one in-flight call needs besides the (read-only) tables: kernel workspace, staging for the host-buffer entry
// points, streams and profiling events.  An encoder keeps a pool of these; every entry point leases one for the duration of the
// call, so host threads sharing one encoder run concurrently, each on its own workspace and streams ("one encoder
// usable from many host threads") -- the reference's instance is likewise safe to share (its only shared mutable state, the LRU
// memo, is locked: LRUCache.cs:61,99).
struct ChunkBufs {   // the chunk entries: chunks per document and their scan's partial sums, the listed long documents, begun units per sub-tile and their scan (+ the total); the host entries' table
    DevBuf ck_cnt, ck_bsum, ck_list, ck_ucnt, ck_ubase, ck_stage;
    void release() { release_each({&ck_cnt, &ck_bsum, &ck_list, &ck_ucnt, &ck_ubase, &ck_stage}); }
};
struct PackBufs {   // the packed entries: the unframed ids and their offsets (framed calls only), segment starts per tile, their scan and its partial sums; the block of a
    // batch without bytes ({T, n_rows, n_segs}, a zero total, a zero error word); the host entries' pos and seg_starts
    DevBuf pk_ids, pk_offs, pk_cnt, pk_base, pk_bsum, pk_tot, pk_stage;
    void release() { release_each({&pk_ids, &pk_offs, &pk_cnt, &pk_base, &pk_bsum, &pk_tot, &pk_stage}); }
};
struct PadBufs {    // the padded entries: the uncut ids and their offsets, the first kept id of every document, the partials of k_pad_lens (kPadGridMax lengths, then
    // as many counts); the block of a batch without bytes ({total, W, n_cut}, a zero total, a zero error word); the host entries' pos, lens and mask
    DevBuf pd_ids, pd_offs, pd_src, pd_part, pd_tot, pd_stage;
    void release() { release_each({&pd_ids, &pd_offs, &pd_src, &pd_part, &pd_tot, &pd_stage}); }
};
struct BktBufs {    // the bucketed entries (beside PadBufs, which they use as the padded entries do): the sort's keys and documents, twice, and lens and src of the
    // sorted rows behind them; the digit counts of every tile and their bases; the block sums of the scans; R_b * W_b and the offsets of every bucket; the host
    // entries' order, rank, widths and offsets
    DevBuf bk_keys, bk_idx, bk_hist, bk_base, bk_bsum, bk_cnt, bk_boffs, bk_stage;
    void release() { release_each({&bk_keys, &bk_idx, &bk_hist, &bk_base, &bk_bsum, &bk_cnt, &bk_boffs, &bk_stage}); }
};
struct TbkBufs {    // the budgeted entries (beside PadBufs and BktBufs, which they use as the bucketed entries do): the marks of every group of 64 sorted rows and
    // their bases; the run table (first row, width, entry row, R_w, regular buckets, the crossing bucket's end, buckets, first bucket: 56 bytes a run); the
    // first row and the width of every bucket below min(n_docs, bucket_cap); {n_buckets, P}, the runs, a spare total; the host entries' bucket rows
    DevBuf tb_marks, tb_runs, tb_rows, tb_fig, tb_stage;
    void release() { release_each({&tb_marks, &tb_runs, &tb_rows, &tb_fig, &tb_stage}); }
};
struct PairBufs {   // the pair entries: the uncut ids and their offsets, the record of every pair (the first kept id of either text, srcA and srcB, then the row's
    // len and the kept count ka of the first text in one word: 24 bytes a pair), the partials of k_pair_lens (kPairGridMax lengths, then as many counts); the block of a batch without bytes
    // ({total, W, n_cut}, a zero total, a zero error word); the host entries' pos, lens, kept, mask and types
    DevBuf pr_ids, pr_offs, pr_src, pr_part, pr_tot, pr_stage;
    void release() { release_each({&pr_ids, &pr_offs, &pr_src, &pr_part, &pr_tot, &pr_stage}); }
};
struct Workspace : SpecialBufs, HostStageBufs, DecodeBufs, DecodeUtf16Bufs, DecodeSmallBufs, PieceBufs, TrimBufs, SpanBufs, ChunkBufs, PackBufs, PadBufs, BktBufs, TbkBufs, PairBufs {
    // kernel workspace
    DevBuf w_gq, w_gcnt, w_xq, w_startbits, w_tmp, w_dense, w_tcount, w_prank, w_pcount, w_pbase, w_tbase, w_bsum, w_doctok, w_dcount, w_dbase, w_pool;
    // what every batch starts from as zeros -- the counter block, the document-start bitmap, the per-sub-tile flags -- lives in ONE buffer, zeroed by ONE
    // memset (three launches were three dependent launches: a batch of a few megabytes is made of little else)
    DevBuf w_zero; size_t zero_bytes = 0;
    DevView w_counters, w_docbits, w_heavyq;
    DevBuf w_mlist, w_mquad, w_mcount, w_pextra, w_coopq, w_lqcnt, w_lqbase, w_lq;
    DevBuf w_counts3;                      // {n_docs, n_bytes, n_tokens} of the batch this workspace is running (tkz_pending_counts_device)
    void release_core() {
        release_each({&w_gq, &w_gcnt, &w_xq, &w_startbits, &w_tmp, &w_dense, &w_tcount, &w_prank, &w_pcount, &w_pbase, &w_tbase, &w_bsum, &w_doctok, &w_dcount, &w_dbase, &w_pool,
                      &w_zero, &w_mlist, &w_mquad, &w_mcount, &w_pextra, &w_coopq, &w_lqcnt, &w_lqbase, &w_lq, &w_counts3});
    }
    U16Stage u16[2];
    bool learn_window_start = false;       // this learning batch opens a window: the hit counters and the log start from zero
    int64_t n_seg = 0;                     // segments of the batch whose marks the workspace holds (w_segoffs)
    int64_t spec_taken = 0;                // literals taken in that batch
    bool sized = false;                    // a batch has run to its end here: the lists and the record buffer have seen real text (encode_device: the sizing attempt)
    int32_t mcap = tkz::kMissCapMin;       // entries of a sub-tile's miss list; grows (once, to what the batch needed) when a sub-tile overflows it
    bool place128 = false;                 // a recent batch of this workspace had more than a fifth of its sub-tiles above 64 list entries: k_place<128>
    int low_lists = 0, low_place = 0;      // consecutive batches that would have done with shorter lists / with k_place<64> (hysteresis: kLowBatches)
    bool learning = false;                 // this workspace's batch counts memo hits per slot (TkzTables::memo_hits): the encoder promotes the hottest entries when it ends
    uint64_t tables_gen = 0;               // AdaptPolicy::generation() when this workspace's batch took its copy of the tables (arm_learning; handed to batch_ended)
    // a pipelined host call runs on TWO leased workspaces: each names the other for the length of the call, and says whether a chunk's launch sequence is in
    // flight on it (HostPipeline; written and read by the call's own thread only -- arm_learning asks it of the asking workspace's sibling and of no other)
    Workspace* sibling = nullptr;
    bool chunk_in_flight = false;
    CounterBlock* h_counters = nullptr;   // pinned
    // the single-launch path for small batches (k_small): input, output and status in ONE page-locked block the device reads and writes directly
    uint8_t* h_small = nullptr;
    bool fork_token = false;               // this workspace's call holds the process's one permission to use the side streams (g_fork_in_flight)
    int64_t forked_batches = 0;            // batches that ran the long pieces' kernels beside k_merge_short (tkz_encoder_side_by_side_batches)
    int64_t last_coop = 0;                 // ... and how many of its long misses were pieces of more than 128 bytes (a wavefront each: k_merge_coop)
    int64_t last_lq_total = -1;            // entries of the class queue of the long misses in the workspace's last batch on the batch path (-1: none yet)
    hipStream_t st_side = nullptr, st_side2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr;   // large batches: k_merge_long_q and k_merge_coop run beside k_merge_short (launch_encode)
    hipStream_t st_small = nullptr;        // (non-blocking: a small call never waits for another thread's batch on the legacy default stream)
    std::atomic<int64_t> small_calls{0}, small_fallbacks{0};   // (read by tkz_encoder_small_path_calls from other threads)
    int64_t small_clocks[16] = {};         // the phase stamps of the last single-launch call, copied out after its synchronisation
    std::atomic<int64_t> dsmall_calls{0}, dsmall_fallbacks{0};   // the same for k_dec_small (tkz_encoder_small_decode_calls)
    int64_t dsmall_clocks[16] = {};
    hipStream_t st_compute = nullptr, st_in = nullptr, st_out = nullptr;   // the host-buffer entry points: kernels / uploads / downloads
    hipEvent_t ev_in[2] = {}, ev_out[3] = {};
    tkz::SdmaSignal sig_out[3], sig_outoffs[3];   // downloads on a copy engine of their own (tkz_sdma.h): the completion signal of each staging set
    int sdma_state = 0;                    // 0 not looked at, 1 in use, -1 not available: the runtime's hipMemcpyAsync
    std::atomic<int64_t> engine_downloads{0};      // copies of results that went by copy engine (tkz_encoder_engine_downloads)
    int64_t bytes_allocated = 0;
    bool busy = false;
    // profiling
    hipEvent_t ev[tkz::K_COUNT][2] = {};
    bool ev_used[tkz::K_COUNT] = {};
    double ms[tkz::K_COUNT] = {};
    int64_t launches[tkz::K_COUNT] = {};
    void release_all() {
        release_core();
        SpecialBufs::release(); HostStageBufs::release(); DecodeBufs::release(); DecodeUtf16Bufs::release(); DecodeSmallBufs::release(); PieceBufs::release(); TrimBufs::release(); SpanBufs::release(); ChunkBufs::release(); PackBufs::release(); PadBufs::release(); BktBufs::release(); TbkBufs::release(); PairBufs::release();
        for (U16Stage& U : u16) U.release();
        if (h_counters) (void)hipHostFree(h_counters);
        if (h_small) (void)hipHostFree(h_small);
        if (st_small) (void)hipStreamDestroy(st_small);
        for (hipStream_t st : {st_side, st_side2}) if (st) (void)hipStreamDestroy(st);
        for (hipEvent_t ev : {ev_fork, ev_join, ev_join2}) if (ev) (void)hipEventDestroy(ev);
        for (int k = 0; k < tkz::K_COUNT; ++k) for (int q = 0; q < 2; ++q) if (ev[k][q]) (void)hipEventDestroy(ev[k][q]);
        for (int q = 0; q < 2; ++q) if (ev_in[q]) (void)hipEventDestroy(ev_in[q]);
        for (int q = 0; q < 3; ++q) if (ev_out[q]) (void)hipEventDestroy(ev_out[q]);
        if (st_compute) (void)hipStreamDestroy(st_compute);
        if (st_in) (void)hipStreamDestroy(st_in);
        if (st_out) (void)hipStreamDestroy(st_out);
        for (int q = 0; q < 3; ++q) { tkz::sdma_signal_destroy(&sig_out[q]); tkz::sdma_signal_destroy(&sig_outoffs[q]); }
    }
};

struct tkz_encoder {
    int device = 0;
    int pattern = 0;
    int max_key_len = 0;
    bool pretok_seq = false;
    bool profiling = false;
    std::mutex mu;                         // the workspace pool, the decoder table
    std::vector<Workspace*> pool;
    // device tables (read-only once built)
    DevBuf t_short, t_mid, t_long, t_blob, t_pair, t_byte, t_bpair, t_bmp, t_counts3, t_memo;
    uint32_t memo_slots = 0;               // the piece memo (tkz_tables.h); TKZ_OPT_PIECE_MEMO switches its use
    TkzTables T{};
    // Decode: id -> bytes (vocabulary keys + registered special tokens), rebuilt when the special tokens change
    DevBuf t_decoff, t_decblob, t_decids;
    TkzDecodeTable D{};
    std::vector<std::pair<int32_t, std::string>> dec_vocab, dec_special;   // host copies (id, bytes)
    // the registered special tokens as the special entries' kernels read them (tkz_kernels.h: TkzLitTable), rebuilt with the decode table.  lit_state: 0 none
    // registered, 1 table built, -1 the set is beyond what the device path holds (lit_why; the special entries answer TKZ_E_UNSUPPORTED)
    DevBuf t_lit;
    tkz::TkzLitTable LIT{};
    int lit_state = 0;
    bool lit_fffd = false;                 // a registered literal holds U+FFFD (TkzLitTable's second 256-bit set is not empty)
    std::string lit_why;
    std::atomic<int64_t> spec_batches{0}, spec_literals{0};                // tkz_encoder_special_stats
    std::atomic<int64_t> packed_calls{0};                                 // tkz_encoder_packed_calls: successful calls of the packed entries
    std::atomic<int64_t> padded_calls{0};                                 // tkz_encoder_padded_calls: successful calls of the padded entries
    std::atomic<int64_t> bucketed_calls{0};                               // tkz_encoder_bucketed_calls: successful calls of the bucketed entries
    std::atomic<int64_t> budgeted_calls{0};                               // tkz_encoder_budgeted_calls: successful calls of the budgeted entries
    std::atomic<int64_t> pairs_calls{0};                                  // tkz_encoder_pairs_calls: successful calls of the pair entries
    std::atomic<int64_t> chunks_overlap_calls{0};                          // tkz_encoder_chunks_overlap_calls: successful calls of the overlap chunk entries
    std::atomic<int64_t> chunks_calls{0};                                  // tkz_encoder_chunks_calls: successful calls of the chunk entries
    std::atomic<int64_t> spans_calls{0};                                   // tkz_encoder_spans_calls: successful calls of the span entries
    std::atomic<int64_t> count_calls{0}, count_single{0};                  // tkz_encoder_count_calls: successful count calls, and those of them that took the single launch
    int64_t bytes_allocated = 0;           // tables
    std::atomic<int64_t> last_xcount{0}, last_xcount2{0};   // tkz_encoder_pretok_leftovers
    bool small_ok = false;                 // the device's LDS per workgroup holds k_small's (kSmallLdsBytesNeeded)
    bool piece_stats = false;              // TKZ_OPT_PIECE_STATS
    int64_t latency_bytes = [] { const char* v = getenv("TKZ_LATENCY_BYTES"); return v ? (int64_t)atoll(v) : int64_t(16) << 20; }();   // TKZ_OPT_LATENCY_BYTES
    bool case_equiv = false;               // TKZ_OPT_CASE_EQUIVALENCE: `'` + U+017F is a contraction under cl100k (a .NET >= 7 host)
    size_t bmp_image_bytes = 0;            // the class table image on the device (t_bmp)
    DevBuf t_stats;                        // its device block (EncodeParams::stats)
    int64_t stat_batches = 0, stat_giants = 0;   // ... and what the host adds per batch (under mu)
    int pending = 0;                       // tkz_pending handles outstanding (under mu)
    bool destroyed = false;                // tkz_encoder_destroy was called while handles were outstanding: the last _end frees the encoder
    // ---- promoted pieces (tkz_tables.h): hot memo entries moved into the SHORT / MID tables themselves.  All under mu. ----
    tkz::AdaptPolicy policy;               // WHEN a window opens, is promoted, is thrown away (tkz_adapt.h); every call to it is made with mu held
    DevBuf t_memo_hits, t_promo;           // the hit counters of a learning batch; the token quads of the promoted pieces
    DevBuf t_long_log;                     // ... and its log of merged pieces of 17..28 bytes (EncodeParams::long_log)
    int64_t long_log_n = 0;                // records the last learning batch left there (set when it ended)
    std::vector<DevBuf> retired;           // table images replaced while other calls may still have been probing them: freed when no call of the encoder is in flight (Lease)
    std::vector<tkz::KeyItem> promo_items; // promoted piece -> promo code, in order of promotion
    std::unordered_set<std::string> promo_keys;
    std::vector<uint32_t> promo_quads;     // 4 tokens per promoted piece (host copy of t_promo)
    uint32_t short_slots_n = 0, mid_slots_n = 0;
    // an automatic promotion runs behind the batch that gathered its statistics (the copy of the memo back to the host, the choice and the rebuilt key
    // tables are ~50 ms of host work: not something the call that happened to be the learning batch should wait for).  The policy's learning slot stays taken until it
    // is done, so there is one at a time; joined by join_promotion()
    std::thread promo_thread;
    std::mutex promo_join_mu;
};

namespace {

// ONE batch at a time in the whole process runs kernels on side streams behind events (launch_encode's forked form): two such batches at once are six streams with
// waits on one another's events, on a runtime that maps streams onto a handful of hardware queues -- a call that finds the permission taken keeps the serial form
std::atomic<int> g_fork_in_flight{0};

// ---- what one call asks for: filled once by its entry point, handed down as it is ----------------------------------------------------------

// A call of one of the special entries: which registered literals it allows (special_call).  It lives in the entry's frame for the length of the call.
struct SpecialCall { tkz::TkzLitAllowed allowed; bool fffd = false; };      // fffd: a registered literal holds U+FFFD (a UTF-16 entry then keeps the replaced-byte bitmap)
// where the piece-granular entry point wants its arrays (all on the device)
struct PiecesOut { int64_t* piece_boffs; int64_t* piece_toffs; int64_t* doc_piece; int64_t piece_cap; int64_t n_pieces; };
// A call of one of the trim entries: the side, the maximum (uniform, or one per document on the device) and where the cut of every document goes (device, may be null)
struct TrimCall { int32_t side; int64_t max_tokens; const int64_t* d_max; int64_t* d_cut_bytes; int64_t* d_cut_units; };
// A call of one of the span entries: where the byte and the UTF-16 unit position of every token go (device, out_cap entries each; either may be null, not both)
struct SpanCall { int32_t* d_tok_bytes; int32_t* d_tok_units; };
// A call of one of the chunk entries: the budget, where the chunk table goes (device; bytes and units may be null) and, on the host, where the number of chunks goes
// overlap >= 0: one of the overlap entries -- the walks of launch_chunks_overlap, the ends of the chunks (d_chunk_ends required, the end positions may be null)
struct ChunkCall {
    int64_t max_tokens; int64_t* d_doc_chunk_offs; int64_t* d_chunk_tokens; int64_t* d_chunk_bytes; int64_t* d_chunk_units; int64_t chunk_cap; int64_t* n_chunks;
    int64_t overlap = -1; int64_t* d_chunk_ends = nullptr; int64_t* d_chunk_end_bytes = nullptr; int64_t* d_chunk_end_units = nullptr;
    bool wants_units() const { return d_chunk_units || d_chunk_end_units; }
};
// A call of one of the packed entries: the framing ids (-1: none), the row length and the pad id, where pos and seg_starts go (device, either may be null) and, on the
// host, where the numbers of rows and segments go
struct PackCall { int32_t bos_id, eos_id; int64_t row_len; int32_t pad_id; int32_t* d_pos; int64_t* d_seg_starts; int64_t seg_cap; int64_t* n_rows; int64_t* n_segs;
                  int64_t frame() const { return (bos_id >= 0) + (eos_id >= 0); } };
// A call of one of the padded entries: the framing ids (-1: none), the maximum length, the two sides, the pad id and the multiple, where the mask, pos and lens go
// (device; mask and pos may be null -- and BatchCall::d_out_offs too) and, on the host, where the width and the number of cut documents go
struct PadCall { int32_t bos_id, eos_id; int64_t max_len; int32_t cut_side, pad_side, pad_id; int64_t pad_multiple; uint8_t* d_mask; int32_t* d_pos; int32_t* d_lens;
                 int64_t* width; int64_t* n_cut; };
// A call of one of the bucketed entries: a PadCall (BatchCall::padded is set as well: its width receives P) and the rows a bucket, the direction, and where the
// permutation, its inverse (may be null) and the bucket table go (device)
struct BktCall { int64_t bucket_rows; int32_t order; int64_t* d_order; int64_t* d_rank; int64_t* d_bucket_offs; int32_t* d_bucket_widths;
                 int64_t buckets(int64_t n_docs) const { return (n_docs + bucket_rows - 1) / bucket_rows; } };
// A call of one of the budgeted entries: a BktCall (BatchCall::bucketed is set as well: bucket_rows is the cap B) and the token budget, the entries of the
// caller's bucket arrays, where the buckets' first rows go (device) and, on the host, where n_buckets goes
struct TbkCall { int64_t token_budget, bucket_cap; int64_t* d_bucket_rows; int64_t* n_buckets;
                 int64_t table_cap(int64_t n_docs) const { return std::min(n_docs, bucket_cap); } };
// A call of one of the pair entries: the framing ids (-1: none), the separator and how many of it, the maximum length, the strategy, the two sides, the pad id and
// the multiple, where the mask, types, pos, lens and kept go (device; all but lens may be null -- and BatchCall::d_out_offs too) and, on the host, where the width
// and the number of cut pairs go
struct PairCall { int32_t bos_id, sep_id, sep_count, eos_id; int64_t max_len; int32_t strategy, cut_side, pad_side, pad_id; int64_t pad_multiple;
                  uint8_t* d_mask; uint8_t* d_types; int32_t* d_pos; int32_t* d_lens; int32_t* d_kept; int64_t* width; int64_t* n_cut; };
// the caller's page-locked text and offsets as the device sees them: encode_device fetches them itself (k_ingest) into d_bytes / d_offs
struct IngestSrc { const uint8_t* h_bytes; const int64_t* h_offs; };

enum class CallKind {
    Encode,          // documents -> pre-tokenizer -> ids, a token offset per document
    OnePiecePerDoc,  // tkz_encode_pieces: no pre-tokenizer, every "document" is one piece
    BitmapOnly,      // tkz_pretokenize_utf8: the piece-start bitmap and nothing else
    Pieces,          // tkz_encode_batch_pieces_utf8: ids, and byte / token offsets of every piece
    Trim,            // tkz_encode_batch_trim_device: Pieces with the piece arrays and the untrimmed ids kept in the workspace, then the cut and the kept ids
    Spans,           // tkz_encode_batch_spans_device: Pieces with the piece arrays in the workspace and the ids in the caller's buffer, then the position of every token
    Chunks,          // tkz_encode_batch_chunks_device: as Spans, then the chunk table
    Packed,          // tkz_encode_batch_packed_device: Encode's own sequence (no piece arrays), then the framed stream laid out in rows, pos and seg_starts
    Padded,          // tkz_encode_batch_padded_device: Encode's own sequence with the ids in the workspace, then a cut, framed and padded row a document
    Bucketed,        // tkz_encode_batch_bucketed_device: as Padded up to the lengths, then the documents sorted by length and a width per bucket of rows
    Budgeted,        // tkz_encode_batch_budgeted_device: as Bucketed up to the sort, then buckets of at most a token budget of positions
    Pairs            // tkz_encode_batch_pairs_device: Encode's own sequence with the ids in the workspace, then a cut, framed and padded row a PAIR of documents
};

// One batch as the device path sees it (encode_device and its stages).  tkz_pending and the chunk pipeline keep the descriptor they began a batch with and hand
// the same one to kCallEnd.
struct BatchCall {
    const uint8_t* d_bytes; const int64_t* d_offs; int64_t n_docs, total;
    int32_t* d_out; int64_t out_cap; int64_t* d_out_offs;
    hipStream_t stream;
    CallKind kind = CallKind::Encode;
    uint64_t* d_bitmap = nullptr;              // BitmapOnly: where the bitmap goes
    PiecesOut* pieces = nullptr;               // Pieces: where the piece arrays go
    const SpecialCall* special = nullptr;      // the special entries (an ordinary encode or a trim call); null: no literal is looked for
    const TrimCall* trim = nullptr;            // Trim: what to keep (pieces then points at the workspace's piece arrays)
    const SpanCall* spans = nullptr;           // Spans: where the positions go (pieces points at the workspace's piece arrays as well)
    const ChunkCall* chunks = nullptr;         // Chunks: the budget and where the table goes (pieces likewise)
    const PackCall* packed = nullptr;          // Packed: the framing, the row length and where pos and seg_starts go
    const PadCall* padded = nullptr;           // Padded, Bucketed: the framing, the cut, the padding and where the mask, pos and lens go
    const BktCall* bucketed = nullptr;         // Bucketed, Budgeted: the rows a bucket, the direction and where the permutation and the bucket table go
    const TbkCall* budgeted = nullptr;         // Budgeted: the token budget, the bucket capacity and where the buckets' first rows go
    const PairCall* pairs = nullptr;           // Pairs: the framing, the separators, the strategy, the padding and where the mask, types, pos, lens and kept go
    int64_t* d_counts3 = nullptr;              // the caller's block for this batch's {n_docs, n_bytes, n_tokens} (may be null)
    const IngestSrc* ingest = nullptr;         // the text is fetched from the caller's page-locked memory by the first attempt
    const uint64_t* d_repl = nullptr;          // the special entries on text transcoded from UTF-16: the replaced-byte bitmap (launch_lit_scan), or null
    bool count_only = false;                   // tkz_count_*: Encode only -- the token offsets and no ids (k_tokcount where k_place stands; d_out null, out_cap 0, never TKZ_E_CAPACITY)
    bool pretokenizes() const { return kind != CallKind::OnePiecePerDoc; }
    bool bitmap_only() const { return kind == CallKind::BitmapOnly; }
    bool plain_encode() const { return kind == CallKind::Encode; }                        // the sizing sample and the special literals are for these
    bool piece_granular() const { return kind == CallKind::Trim || kind == CallKind::Spans || kind == CallKind::Chunks; }      // (Pieces with the piece arrays in the workspace)
    bool may_learn() const { return pretokenizes() && !bitmap_only(); }                   // pre-tokenized text that reaches the key tables
    const SpecialCall* literals() const { return plain_encode() || piece_granular() || kind == CallKind::Packed || kind == CallKind::Padded || kind == CallKind::Bucketed || kind == CallKind::Budgeted || kind == CallKind::Pairs ? special : nullptr; }
};

// tkz_encode_trim_utf8 / _utf16 (ONE text, cut to a maximum): the side, the maximum and where the cut's lengths go (host memory; either may be null)
struct TrimOne { int32_t side; int64_t max_tokens; int64_t* cut_bytes; int64_t* cut_units; };

// One batch in the caller's host memory, as the host entries hand it to encode_host.
struct HostCall {
    const uint8_t* bytes; const uint16_t* units;       // UTF-8 bytes, or (utf16) UTF-16 code units (offsets in units then)
    const int64_t* offs; int64_t n_docs;
    int32_t* out_ids; int64_t out_cap; int64_t* out_offsets; int64_t* needed;
    CallKind kind = CallKind::Encode;                  // (never Pieces: that entry stages its own buffers)
    uint64_t* bitmap = nullptr;                        // BitmapOnly: the caller's words
    const SpecialCall* special = nullptr;
    bool utf16 = false;
    // tkz_encode_special_utf8 / _utf16 (ONE text, special tokens): the only special calls that may take the single-launch path.  small_form: null, or (the UTF-16
    // one) the same text transcoded on the host, which that path takes in the place of this call; repl: its replaced-byte bitmap, or null (utf16_to_utf8)
    bool single = false;
    const HostCall* small_form = nullptr;
    const uint64_t* repl = nullptr;
    // the single-text trim entries: the single-launch path runs its trim form, out_cap counts the KEPT ids and *needed receives their count
    const TrimOne* trim = nullptr;
    // tkz_count_*: the offsets and no ids (out_ids null, out_cap 0); *took_single: null, or set when the single-launch kernel answered the call
    bool count_only = false;
    bool* took_single = nullptr;
    bool u16() const { return utf16; }
    int64_t total() const { return offs[n_docs]; }     // bytes, or code units
    bool plain_encode() const { return kind == CallKind::Encode; }
    // the same call on device buffers
    BatchCall on_device(const uint8_t* d_bytes, const int64_t* d_offs, int64_t nd, int64_t nbytes, int32_t* d_out, int64_t cap, int64_t* d_out_offs, hipStream_t stream) const {
        BatchCall c{d_bytes, d_offs, nd, nbytes, d_out, cap, d_out_offs, stream};
        c.kind = kind; c.special = special; c.count_only = count_only;
        return c;
    }
};

// a workspace of the encoder's pool for the duration of one call
struct Lease {
    tkz_encoder* e; Workspace* ws = nullptr;
    explicit Lease(tkz_encoder* enc) : e(enc) {
        std::lock_guard<std::mutex> lock(e->mu);
        for (Workspace* w : e->pool) if (!w->busy) { ws = w; break; }
        if (!ws) { ws = new Workspace(); e->pool.push_back(ws); }
        ws->busy = true;
    }
    ~Lease() {
        std::lock_guard<std::mutex> lock(e->mu);
        if (ws->fork_token) { ws->fork_token = false; g_fork_in_flight.store(0); }
        ws->busy = false;
        // table images a promotion replaced: every call takes its copy of the table descriptor while it holds a workspace, so with no workspace leased
        // nothing can be probing them any more
        if (!e->retired.empty()) {
            for (Workspace* w : e->pool) if (w->busy) return;
            for (DevBuf& b : e->retired) { e->bytes_allocated -= (int64_t)b.cap; b.release(); }
            e->retired.clear();
        }
    }
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
};

void prof_hook(void* ctx, int id, int phase, hipStream_t s) {
    Workspace* e = static_cast<Workspace*>(ctx);
    if (!e->ev[id][phase]) (void)hipEventCreate(&e->ev[id][phase]);
    (void)hipEventRecord(e->ev[id][phase], s);
    if (phase == 1) e->ev_used[id] = true;
}
void prof_collect(Workspace* e) {
    for (int k = 0; k < tkz::K_COUNT; ++k) {
        if (!e->ev_used[k]) continue;
        float t = 0;
        if (hipEventElapsedTime(&t, e->ev[k][0], e->ev[k][1]) == hipSuccess) { e->ms[k] += t; e->launches[k] += 1; }
        e->ev_used[k] = false;
    }
}

template <class T>
hipError_t upload(DevBuf& b, const std::vector<T>& v, int64_t* acc) {
    hipError_t e = b.ensure(std::max<size_t>(16, v.size() * sizeof(T)), acc);
    if (e != hipSuccess) return e;
    return hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// (re)builds the device decoder table from the vocabulary keys and the registered special tokens.  The reference looks an id
// up in Decoder first, then in SpecialTokensDecoder (TikTokenizer.cs:591-598): a special token never shadows a vocabulary id.
tkz_status build_decode_table(tkz_encoder* e) {
    std::vector<std::pair<int32_t, const std::string*>> ent;
    ent.reserve(e->dec_vocab.size() + e->dec_special.size());
    for (const auto& kv : e->dec_vocab) ent.emplace_back(kv.first, &kv.second);
    const size_t nv = ent.size();
    for (const auto& kv : e->dec_special) ent.emplace_back(kv.first, &kv.second);
    // stable by id: of two entries with one id the vocabulary's (first) wins
    std::vector<size_t> order(ent.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return ent[a].first < ent[b].first; });
    (void)nv;
    int64_t max_id = -1;
    for (const auto& kv : ent) max_id = std::max<int64_t>(max_id, kv.first);
    const bool dense = max_id < (int64_t(1) << 22);
    std::vector<uint32_t> off;
    std::vector<int32_t> ids;
    std::vector<uint8_t> blob;
    if (dense) {
        off.assign((size_t)(max_id + 2), 0);
        std::vector<const std::string*> by_id((size_t)(max_id + 1), nullptr);
        for (size_t k : order) if (ent[k].first >= 0 && !by_id[(size_t)ent[k].first]) by_id[(size_t)ent[k].first] = ent[k].second;
        for (int64_t i = 0; i <= max_id; ++i) {
            off[(size_t)i] = (uint32_t)blob.size();
            if (by_id[(size_t)i]) blob.insert(blob.end(), by_id[(size_t)i]->begin(), by_id[(size_t)i]->end());
        }
        off[(size_t)(max_id + 1)] = (uint32_t)blob.size();
    } else {
        int64_t last = INT64_MIN;
        for (size_t k : order) {
            if (ent[k].first == last) continue;
            last = ent[k].first;
            ids.push_back(ent[k].first);
            off.push_back((uint32_t)blob.size());
            blob.insert(blob.end(), ent[k].second->begin(), ent[k].second->end());
        }
        off.push_back((uint32_t)blob.size());
    }
    blob.resize(blob.size() + 16, 0);
    int64_t* acc = &e->bytes_allocated;
    hipError_t h = upload(e->t_decoff, off, acc);
    if (h == hipSuccess) h = upload(e->t_decblob, blob, acc);
    if (h == hipSuccess && !dense) h = upload(e->t_decids, ids, acc);
    if (h != hipSuccess) return fail(TKZ_E_DEVICE, std::string("decoder table upload: ") + hipGetErrorString(h));
    e->D.off = e->t_decoff.as<uint32_t>(); e->D.blob = e->t_decblob.as<uint8_t>(); e->D.ids = dense ? nullptr : e->t_decids.as<int32_t>();
    e->D.n = dense ? max_id + 1 : (int64_t)ids.size(); e->D.dense = dense ? 1 : 0;
    return TKZ_OK;
}

// ---- promoted pieces ------------------------------------------------------------------------------------------------------------------------
// The reference's LRUCache (TikTokenizer.cs:254,270) answers a piece it has seen before without running BytePairEncode again; the device memo does
// the same inside k_merge_short -- at the price of a list entry, a quad, a 32-byte slot and an answer per missed piece and batch.  Under a
// vocabulary that has not seen the text 7 of 8 short misses are such hits and that kernel is 40 % of the step.  A memo answer never changes, so the
// hottest ones are PROMOTED: the host reads the memo (and, after a learning batch, the sampled hit count of every slot) back, adds the pieces to the
// SHORT / MID key tables with a promo code in place of a rank (tkz_tables.h), and uploads the new images; k_probe then finds such a piece like any
// key, the merge kernels never see it, k_place gathers its <= 4 tokens.  Results are the same ids by construction (the memo's answers are exact and a
// slot is read back under the same validity rule the kernels use); the tests compare a promoted encoder with the oracle.
constexpr int64_t kLongLogCap = 65536;             // records of merged 17..28-byte pieces a learning batch may log (EncodeParams::long_log)

// (re)builds the SHORT / MID images from the vocabulary's keys + the promoted pieces and publishes them; `retire`: other calls may be probing the
// current images (they are kept until the encoder is destroyed), else they are freed
// The registered special tokens as k_lit_scan / k_probe_special read them (called with e->mu held, behind build_decode_table).  A set the device path does not
// hold -- more than 256 literals, one that is empty, longer than 128 bytes or not well-formed UTF-8 (a segment mark would fall inside a character), an id a piece
// record cannot carry beside its flag bits and the promoted pieces' codes -- is no error here (Decode takes any): the special entries then answer TKZ_E_UNSUPPORTED.
bool well_formed_utf8(const std::string& t) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(t.data());
    const size_t n = t.size();
    for (size_t i = 0; i < n;) {
        const unsigned c = b[i];
        int len; uint32_t cp, lo;
        if (c < 0x80) { ++i; continue; }
        else if ((c & 0xE0) == 0xC0) { len = 2; cp = c & 0x1F; lo = 0x80; }
        else if ((c & 0xF0) == 0xE0) { len = 3; cp = c & 0x0F; lo = 0x800; }
        else if ((c & 0xF8) == 0xF0) { len = 4; cp = c & 0x07; lo = 0x10000; }
        else return false;
        if (i + len > n) return false;
        for (int k = 1; k < len; ++k) { if ((b[i + k] & 0xC0) != 0x80) return false; cp = (cp << 6) | (b[i + k] & 0x3F); }
        if (cp < lo || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
        i += len;
    }
    return true;
}
tkz_status build_literal_table(tkz_encoder* e) {
    using namespace tkz;
    e->LIT = TkzLitTable{};
    e->lit_state = 0;
    e->lit_fffd = false;
    e->lit_why.clear();
    const auto& sp = e->dec_special;
    if (sp.empty()) return TKZ_OK;
    auto refuse = [&](const std::string& why) { e->lit_state = -1; e->lit_why = why; return TKZ_OK; };
    if (sp.size() > (size_t)kLitMax) return refuse("more than 256 special tokens are registered");
    std::vector<uint32_t> img((size_t)kLitMetaHead + 2 * sp.size(), 0u);
    std::string blob;
    for (size_t i = 0; i < sp.size(); ++i) {
        const std::string& lit = sp[i].second;
        if (lit.empty()) return refuse("an empty special-token literal is registered");
        if (lit.size() > (size_t)kLitMaxLen) return refuse("a special-token literal of more than 128 bytes is registered");
        if (!well_formed_utf8(lit)) return refuse("a special-token literal that is not well-formed UTF-8 is registered");
        if (sp[i].first < 0 || (uint32_t)sp[i].first >= kPromoFlag) return refuse("a special-token id outside [0, 2^26) is registered: a piece record cannot hold it");
        const unsigned c = (unsigned char)lit[0];
        img[c >> 5] |= 1u << (c & 31);
        if (lit.find("\xEF\xBF\xBD") != std::string::npos) { img[kLitFffdHead + (i >> 5)] |= 1u << (i & 31); e->lit_fffd = true; }
        img[kLitMetaHead + 2 * i] = (uint32_t)blob.size() | ((uint32_t)lit.size() << 16);
        img[kLitMetaHead + 2 * i + 1] = (uint32_t)sp[i].first;
        blob += lit;
    }
    const size_t meta_dwords = img.size();
    img.resize(meta_dwords + (blob.size() + 3) / 4, 0u);
    memcpy(img.data() + meta_dwords, blob.data(), blob.size());
    HIP_TRY(upload(e->t_lit, img, &e->bytes_allocated));
    e->LIT.meta = e->t_lit.as<uint32_t>();
    e->LIT.blob = reinterpret_cast<const uint8_t*>(e->t_lit.as<uint32_t>() + meta_dwords);
    e->LIT.n = (int32_t)sp.size();
    e->LIT.blob_bytes = (int32_t)blob.size();
    e->lit_state = 1;
    return TKZ_OK;
}

struct KeyTablesImage { DevBuf nt, np; size_t short_bytes = 0, n_short_slots = 0, n_mid_slots = 0, n_promo = 0; uint32_t sseed = 0, mseed = 0; };
// the images on the device, built from the vocabulary's keys + `promo_items` (copies: no lock is held here, the build takes tens of milliseconds)
tkz_status build_key_tables_image(tkz_encoder* e, const std::vector<tkz::KeyItem>& promo_items, const std::vector<uint32_t>& promo_quads, KeyTablesImage* img) {
    std::vector<tkz::KeyItem> items;
    items.reserve(e->dec_vocab.size() + promo_items.size());
    {   // (dec_vocab's vocabulary part never changes after tkz_encoder_create)
        std::vector<size_t> order(e->dec_vocab.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return e->dec_vocab[a].first < e->dec_vocab[b].first; });      // rank order: most frequent first
        for (size_t i : order) { const std::string& k = e->dec_vocab[i].second; if (!k.empty() && k.size() <= TKZ_MID_KEY_MAX) items.push_back(tkz::KeyItem{k, (uint32_t)e->dec_vocab[i].first}); }
    }
    for (const tkz::KeyItem& it : promo_items) items.push_back(it);
    std::vector<TkzShortSlot> ss; std::vector<TkzMidSlot> ms;
    tkz::build_key_tables(items, &ss, &img->sseed, &ms, &img->mseed);
    const size_t short_bytes = ss.size() * sizeof(TkzShortSlot), mid_bytes = ms.size() * sizeof(TkzMidSlot);
    int64_t acc = 0;
    // (uploads on a stream of their own: on the null stream they would queue behind the batches the host has in flight there)
    hipStream_t cs = nullptr;
    hipError_t h = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
    if (h == hipSuccess) h = img->nt.ensure(std::max<size_t>(64, short_bytes + mid_bytes), &acc);
    if (h == hipSuccess && short_bytes) h = hipMemcpyAsync(img->nt.p, ss.data(), short_bytes, hipMemcpyHostToDevice, cs);
    if (h == hipSuccess && mid_bytes) h = hipMemcpyAsync(static_cast<char*>(img->nt.p) + short_bytes, ms.data(), mid_bytes, hipMemcpyHostToDevice, cs);
    if (h == hipSuccess) h = img->np.ensure(std::max<size_t>(64, promo_quads.size() * 4), &acc);
    if (h == hipSuccess && !promo_quads.empty()) h = hipMemcpyAsync(img->np.p, promo_quads.data(), promo_quads.size() * 4, hipMemcpyHostToDevice, cs);
    if (h == hipSuccess) h = hipStreamSynchronize(cs);
    if (cs) (void)hipStreamDestroy(cs);
    if (h != hipSuccess) { img->nt.release(); img->np.release(); return fail(TKZ_E_DEVICE, std::string("promoted tables: ") + hipGetErrorString(h)); }
    img->short_bytes = short_bytes; img->n_short_slots = ss.size(); img->n_mid_slots = ms.size(); img->n_promo = promo_items.size();
    return TKZ_OK;
}
// ... and put in place (e->mu held).  `retire`: other calls may be probing the current images (kept until the encoder is destroyed), else they are freed
void install_key_tables(tkz_encoder* e, KeyTablesImage& img, bool retire) {
    int64_t* acc = &e->bytes_allocated;
    *acc += (int64_t)(img.nt.cap + img.np.cap);
    if (retire) { e->retired.push_back(e->t_short); e->retired.push_back(e->t_promo); }
    else { *acc -= (int64_t)(e->t_short.cap + e->t_promo.cap); e->t_short.release(); e->t_promo.release(); }
    e->t_short = img.nt; e->t_promo = img.np;
    e->T.short_slots = e->t_short.as<TkzShortSlot>(); e->T.short_nb = (uint32_t)(img.n_short_slots / 2); e->T.short_seed = img.sseed;
    e->T.mid_slots = reinterpret_cast<const TkzMidSlot*>(e->t_short.as<char>() + img.short_bytes); e->T.mid_ns = (uint32_t)img.n_mid_slots; e->T.mid_seed = img.mseed;
    e->T.promo = img.n_promo ? e->t_promo.as<uint4>() : nullptr; e->T.promo_n = (uint32_t)img.n_promo;
    e->short_slots_n = (uint32_t)img.n_short_slots; e->mid_slots_n = (uint32_t)img.n_mid_slots;
    e->policy.tables_replaced();        // (batches that took their copy of e->T before this ran on the tables before: AdaptPolicy::batch_ended)
}

// waits for the automatic promotion in the background, if any (never with e->mu held: the promotion takes it)
void join_promotion(tkz_encoder* e) {
    std::lock_guard<std::mutex> lock(e->promo_join_mu);
    if (e->promo_thread.joinable()) e->promo_thread.join();
}
// The memo (and the hit counters of a learning batch, or null: every valid entry counts alike) is read back and its hottest entries are promoted.
// Called with no lock held; takes e->mu for the bookkeeping and the publication.  *added: entries promoted by this call.
tkz_status promote_from_memo(tkz_encoder* e, bool use_hits, bool retire, int64_t* added) {
    using tkz::kLongLogDwords; using tkz::kLongLogMaxLen;
    if (added) *added = 0;
    if (!e->memo_slots || e->T.max_rank >= (int32_t)kPromoFlag) return TKZ_OK;      // (a promo code must not look like a rank)
    std::vector<TkzMemoSlot> memo(e->memo_slots);
    std::vector<uint32_t> hits;
    // (a stream of its own: this may be the background thread of an automatic promotion, and a copy on the null stream would wait for -- and hold up --
    //  whatever the host has queued there)
    hipStream_t cs = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } stream_guard{cs};
    HIP_TRY(hipMemcpyAsync(memo.data(), e->t_memo.p, memo.size() * sizeof(TkzMemoSlot), hipMemcpyDeviceToHost, cs));
    if (use_hits) { hits.resize(e->memo_slots); HIP_TRY(hipMemcpyAsync(hits.data(), e->t_memo_hits.p, hits.size() * 4, hipMemcpyDeviceToHost, cs)); }
    HIP_TRY(hipStreamSynchronize(cs));
    // ... and the pieces of 17..28 bytes k_merge_long logged during the learning batch (each with its <= 4 tokens): select_promotions
    std::vector<uint32_t> llog;
    if (use_hits && e->t_long_log.p) {      // (the log's record count lives behind the records: it runs on through the batches of a learning window)
        unsigned long long n = 0;
        HIP_TRY(hipMemcpyAsync(&n, e->t_long_log.as<char>() + (size_t)kLongLogCap * kLongLogDwords * 4, 8, hipMemcpyDeviceToHost, cs));
        HIP_TRY(hipStreamSynchronize(cs));
        e->long_log_n = (int64_t)std::min<unsigned long long>(n, (unsigned long long)kLongLogCap);
    }
    if (use_hits && e->long_log_n > 0) {
        llog.resize((size_t)e->long_log_n * kLongLogDwords);
        HIP_TRY(hipMemcpyAsync(llog.data(), e->t_long_log.p, llog.size() * 4, hipMemcpyDeviceToHost, cs));
        HIP_TRY(hipStreamSynchronize(cs));
    }
    std::vector<tkz::KeyItem> items_copy;
    std::vector<uint32_t> quads_copy;
    {
        std::lock_guard<std::mutex> lock(e->mu);
        const tkz::PromoSelection sel = tkz::select_promotions(memo, use_hits ? &hits : nullptr, llog, e->policy.cap(), &e->promo_items, &e->promo_keys, &e->promo_quads);
        if (use_hits) e->policy.memo_read_back(sel.valid_slots, e->memo_slots);
        if (added) *added = sel.added;
        if (!sel.added) return TKZ_OK;
        items_copy = e->promo_items; quads_copy = e->promo_quads;
    }
    // the key tables with the promoted pieces in them: built and uploaded WITHOUT the lock (tens of milliseconds), then put in place under it (only one
    // promotion runs at a time -- the encoder's one learning slot, or an idle encoder --, so the list has not changed in between)
    KeyTablesImage img;
    const tkz_status bs = build_key_tables_image(e, items_copy, quads_copy, &img);
    if (bs != TKZ_OK) return bs;
    std::lock_guard<std::mutex> lock(e->mu);
    install_key_tables(e, img, retire);
    return TKZ_OK;
}

// every promotion dropped: the key tables as the vocabulary alone gives them.  `retire`: see install_key_tables.  No lock held on entry.
tkz_status drop_promotions(tkz_encoder* e, bool retire) {
    {
        std::lock_guard<std::mutex> lock(e->mu);
        if (e->promo_items.empty()) return TKZ_OK;
    }
    KeyTablesImage img;
    const tkz_status st = build_key_tables_image(e, {}, {}, &img);
    if (st != TKZ_OK) return st;
    std::lock_guard<std::mutex> lock(e->mu);
    e->promo_items.clear(); e->promo_keys.clear(); e->promo_quads.clear();
    install_key_tables(e, img, retire);
    return TKZ_OK;
}

// workspace of one batch of `total` bytes / n_docs documents (grow-only buffers: nothing happens once they are large enough)
tkz_status prepare_workspace(Workspace* ws, int64_t total, int64_t n_docs, CallKind kind) {
    using namespace tkz;
    const bool bitmap_only = kind == CallKind::BitmapOnly, pieces = kind == CallKind::Pieces || kind == CallKind::Trim || kind == CallKind::Spans || kind == CallKind::Chunks;
    const int64_t nwords = total / 64 + 1;
    const int64_t ntiles = (total + kSub - 1) / kSub;
    const int64_t nblk = (ntiles + kScanBlock - 1) / kScanBlock;
    int64_t* acc = &ws->bytes_allocated;
    {   // [counter block, 256 B] [document-start bits, nwords + 8 words] [a flag per sub-tile, ntiles + 64 bytes]: zeroed together
        static_assert(sizeof(CounterBlock) <= 256, "the counter block's place in the zero region");
        const size_t off_bits = 256, off_flags = off_bits + (size_t)(nwords + 8) * 8, end = off_flags + (size_t)ntiles + 64;
        HIP_TRY(ws->w_zero.ensure(end, acc));
        ws->w_counters.p = ws->w_zero.p; ws->w_docbits.p = ws->w_zero.as<char>() + off_bits; ws->w_heavyq.p = ws->w_zero.as<char>() + off_flags;
        ws->zero_bytes = bitmap_only ? off_flags : end;
    }
    HIP_TRY(ws->w_startbits.ensure((size_t)(nwords + 8) * 8, acc));
    HIP_TRY(ws->w_counts3.ensure(32, acc));
    if (!bitmap_only) {
        HIP_TRY(ws->w_tmp.ensure((size_t)(total + 64) * 4, acc));
        HIP_TRY(ws->w_dense.ensure((size_t)(ntiles / kMergeGroup + 1) * kDenseCap * 4, acc));
        HIP_TRY(ws->w_tcount.ensure((size_t)ntiles * 4, acc));
        HIP_TRY(ws->w_pcount.ensure((size_t)ntiles * 4, acc));
        HIP_TRY(ws->w_pbase.ensure((size_t)ntiles * 8, acc));
        // one 4-byte record per piece.  The number of pieces is known only after the pre-tokenizer has run (English/code text: a
        // piece per ~4.5 bytes; the bound is a piece per byte): the buffer starts at a piece per 3 bytes, k_probe refuses to write
        // past it, and the batch is redone once with the exact size if that was not enough
        // (+ 8 per sub-tile on average: every sub-tile's records start on a 64-byte line of their own)
        HIP_TRY(ws->w_prank.ensure((size_t)(total / 3 + 8 * ntiles + 4096) * 4, acc));
        HIP_TRY(ws->w_mlist.ensure((size_t)ntiles * (size_t)ws->mcap * 4, acc));
        HIP_TRY(ws->w_mquad.ensure((size_t)ntiles * (size_t)ws->mcap * 16, acc));
        HIP_TRY(ws->w_mcount.ensure((size_t)ntiles * 4, acc));
        HIP_TRY(ws->w_pextra.ensure((size_t)ntiles * 4, acc));
        HIP_TRY(ws->w_coopq.ensure((size_t)(total / kLanePiece + 64) * 8, acc));
        {   // the class queue of the long misses (a long miss is 17 bytes at least): counts and bases per (class, chunk of 64 sub-tiles), 8 bytes an entry
            const int64_t nchunks = (ntiles + 63) / 64;
            HIP_TRY(ws->w_lqcnt.ensure((size_t)nchunks * 16 * 4, acc));
            HIP_TRY(ws->w_lqbase.ensure((size_t)(nchunks * 16 + 1) * 8, acc));
            HIP_TRY(ws->w_lq.ensure((size_t)(total / (kShortMax + 1) + 64) * 8, acc));
        }
        HIP_TRY(ws->w_tbase.ensure((size_t)(ntiles + 1) * 8, acc));
        HIP_TRY(ws->w_bsum.ensure((size_t)(nblk + 1) * 8, acc));
        HIP_TRY(ws->w_doctok.ensure((size_t)((pieces ? total : n_docs) + 2) * 4, acc));    // (piece mode: one entry per piece)
        HIP_TRY(ws->w_dcount.ensure((size_t)ntiles * 4, acc));
        HIP_TRY(ws->w_dbase.ensure((size_t)ntiles * 8, acc));
        HIP_TRY(ws->w_gq.ensure((size_t)(total / kArenaPiece + 2) * 24, acc));     // {position, length} per giant piece + the order they are taken in
        HIP_TRY(ws->w_gcnt.ensure((size_t)ntiles * 4, acc));
        if (!ws->w_pool.p) HIP_TRY(ws->w_pool.ensure((size_t)std::min<int64_t>(24 * total + 4096, int64_t(64) << 20), acc));
    }
    return TKZ_OK;
}

struct SlowCallLog {
    int64_t total; int attempts = 0; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    SlowCallLog(int64_t n) : total(n) { g_alloc_ns = 0; g_alloc_calls = 0; }
    ~SlowCallLog() {
        const char* v = getenv("TKZ_LOG_SLOW_MS");
        const long limit_ms = v ? atol(v) : -1L;
        if (limit_ms < 0) return;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms > (double)limit_ms)
            { fprintf(stderr, "tkz: batch call of %lld bytes: %.1f ms on the host, %.1f ms of it in %d hipMalloc/hipFree calls, %d attempt(s)\n", (long long)total, ms, (double)g_alloc_ns * 1e-6, g_alloc_calls, attempts); fflush(stderr); }
    }
};
// ($TKZ_TRACE_HOST: the host's side of the chunk pipeline on stderr -- microseconds since the pipeline started at which each step RETURNED; development)
struct HostTrace {
    static bool on() { static const bool v = getenv("TKZ_TRACE_HOST") != nullptr; return v; }
    std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
    std::vector<std::pair<std::string, double>> stamps;
    void stamp(const char* what, int64_t k) {
        if (on()) stamps.emplace_back(std::string(what) + " " + std::to_string(k), std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_call).count());
    }
    void print(int64_t nchunks) const {
        if (!on()) return;
        std::string line = "[tkz host trace] " + std::to_string(nchunks) + " chunks:";
        for (const auto& sp : stamps) { char b[96]; snprintf(b, sizeof b, " %s @%.0f", sp.first.c_str(), sp.second); line += b; }
        fprintf(stderr, "%s\n", line.c_str());
    }
};
enum { kCallWhole = 0, kCallBegin = 1, kCallEnd = 2 };
// ---- the stages of one attempt of encode_device ---------------------------------------------------------------------------------------

// a large batch: two more streams, for the two kernels of the long pieces that last as long as their slowest wavefront (launch_encode runs them beside k_merge_short;
// without the streams -- the runtime refused one, or an event -- they follow it as they always did).
// WHEN: the workspace's previous batch left a class queue short enough for its kernel to be a matter of latency -- at most kForkMaxLong entries, ~4 batches of 64 for
// each of the 4,096 wavefronts the chip holds --; with a long queue (mixed text: 17 M entries in 1 GB) the queue kernel is the step's largest and needs the whole chip
// (measured with the tail grids: 17.0 -> 19.8 ms), and on the bench text (1.3 M) the two forms are equal (20.6 / 20.8 ms).
constexpr int64_t kForkMaxLong = int64_t(1) << 20;
// (round 6, last session) ... or up to twice that many when one in 2,048 of them is a piece of more than 128 bytes: such a queue ends in a tail of slow wavefronts
// whatever its length.  436 MB of source text (1.18 M long misses, 1,467 of them of 129+ bytes): 94.5 -> 104.3 GB/s side by side; the bench text (1.31-1.43 M, none
// above 128 bytes) loses 0.1-0.3 ms that way and stays serial.  profiles/r06/variants_side_by_side2.txt
constexpr int64_t kForkMaxLongTail = int64_t(1) << 21, kForkTailShare = 2048;
void side_streams(tkz_encoder* e, Workspace* ws, int64_t total, tkz::Launch* L) {
    const bool short_queue = ws->last_lq_total >= 0 && (ws->last_lq_total <= kForkMaxLong || (ws->last_lq_total <= kForkMaxLongTail && ws->last_coop * kForkTailShare >= ws->last_lq_total));
    if (total <= e->latency_bytes || !short_queue) return;
    if (!ws->fork_token) { int none = 0; ws->fork_token = g_fork_in_flight.compare_exchange_strong(none, 1); }      // (given back when the call ends: ~Lease)
    bool ok = ws->fork_token;
    for (hipStream_t* st : {&ws->st_side, &ws->st_side2}) if (!*st && hipStreamCreateWithFlags(st, hipStreamNonBlocking) != hipSuccess) { *st = nullptr; ok = false; }
    for (hipEvent_t* ev : {&ws->ev_fork, &ws->ev_join, &ws->ev_join2}) if (!*ev && hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess) { *ev = nullptr; ok = false; }
    if (ok) { L->side = ws->st_side; L->side2 = ws->st_side2; L->ev_fork = ws->ev_fork; L->ev_join = ws->ev_join; L->ev_join2 = ws->ev_join2; }
    else (void)hipGetLastError();
}

// THE SIZING ATTEMPT: a fresh workspace's first large batch probes a sixteenth of its sub-tiles first.  How long the miss lists must be (and, from the
// scan, how many records there are) is known after ~1 ms instead of after a whole attempt up to k_probe that is thrown away: a fresh encoder's first
// batch of text its vocabulary has not seen (5.1 GB, held-out vocabulary) went from 100 ms to ~50.  The full attempt follows on the same bitmaps; a
// sample that under-estimates leaves the ordinary retry.  Returns the sub-tiles of the sample, or -1: the batch is too small for a sizing attempt.
int64_t sizing_sample(int64_t ntiles) {
    int64_t min_sub = (int64_t(64) << 20) / tkz::kSub;                      // (64 MB of text; TKZ_SIZING_MIN_SUB: the tests' handle on it)
    { const char* v = getenv("TKZ_SIZING_MIN_SUB"); if (v && atoll(v) > 0) min_sub = atoll(v); }
    return ntiles >= min_sub ? std::min<int64_t>(ntiles, std::max<int64_t>(ntiles / 16, min_sub / 16)) : -1;
}

// The tables as they are NOW, one consistent copy for the whole attempt (a promotion at the end of another call's batch replaces the SHORT / MID images and
// the promo array together: k_probe and k_place of one attempt must see the same generation) -- and whether this batch counts the memo's hits.
tkz_status arm_learning(tkz_encoder* e, Workspace* ws, const BatchCall& c, bool first, TkzTables* T) {
    using namespace tkz;
    const int64_t total = c.total;
    const hipStream_t stream = c.stream;
    {
        std::lock_guard<std::mutex> lock(e->mu);
        // (another call: a leased workspace that is not this call's -- its own sibling counts only while a chunk is in flight on it; that mark is the owning
        //  call's, written without the lock: read for the sibling and for no other workspace)
        bool others = false;
        for (Workspace* w : e->pool) if (AdaptPolicy::other_call_in_flight(w->busy, w == ws, w == ws->sibling, w == ws->sibling && w->chunk_in_flight)) others = true;
        const AdaptPolicy::Arm arm = e->policy.may_learn(total, first && !ws->learning, c.may_learn(), e->T.memo_n != 0, e->T.max_rank < (int32_t)kPromoFlag, e->promo_items.size(), others);
        if (arm != AdaptPolicy::Arm::No && e->t_memo_hits.ensure((size_t)e->memo_slots * 4, &e->bytes_allocated) == hipSuccess &&
            e->t_long_log.ensure((size_t)kLongLogCap * kLongLogDwords * 4 + 64, &e->bytes_allocated) == hipSuccess) {
            // (the memo is cleared under nobody's feet, synchronously, with the encoder's lock held: 16 MB, microseconds, once per drift)
            const bool clear = arm == AdaptPolicy::Arm::YesClearMemo;
            if (!clear || (hipMemsetAsync(e->t_memo.p, 0, size_t(e->memo_slots) * sizeof(TkzMemoSlot), stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess)) {
                ws->learn_window_start = e->policy.window_armed(clear);
                ws->learning = true;
            }
        }
        *T = e->T;
        ws->tables_gen = e->policy.generation();
    }
    if (ws->learning) {
        T->memo_hits = e->t_memo_hits.as<uint32_t>();
        T->memo_hits_sparse = total >= (int64_t(64) << 20) ? 1u : 0u;       // (below 64 MB every hit is counted: a few million atomics at most)
        if (ws->learn_window_start && first) {                              // (a window's later batches add to its counters and its log)
            HIP_TRY(hipMemsetAsync(T->memo_hits, 0, (size_t)e->memo_slots * 4, stream));
            HIP_TRY(hipMemsetAsync(e->t_long_log.as<char>() + (size_t)kLongLogCap * kLongLogDwords * 4, 0, 64, stream));
        }
    }
    return TKZ_OK;
}

// the workspace's buffers as the kernels see them (the batch path and the single-launch kernel alike)
tkz::EncodeParams bind_params(Workspace* ws, const uint8_t* d_bytes, const int64_t* d_offs, int64_t n_docs, int64_t total) {
    using namespace tkz;
    char* cb = ws->w_counters.as<char>();
    EncodeParams P{};
    P.bytes = d_bytes; P.total = total; P.startbits = ws->w_startbits.as<uint64_t>(); P.docbits = ws->w_docbits.as<uint64_t>(); P.nwords = total / 64 + 1;
    P.offs = d_offs; P.n_docs = n_docs;
    P.tmp = ws->w_tmp.as<int32_t>(); P.dense = ws->w_dense.as<int32_t>(); P.tile_count = ws->w_tcount.as<int32_t>();
    P.prank = ws->w_prank.as<int32_t>(); P.prank_cap = (int64_t)(ws->w_prank.cap / 4); P.pcount = ws->w_pcount.as<int32_t>(); P.pbase = ws->w_pbase.as<int64_t>();
    P.mlist = ws->w_mlist.as<uint32_t>(); P.mquad = ws->w_mquad.as<uint4>(); P.mcap = ws->mcap; P.mcount = ws->w_mcount.as<uint32_t>();
    P.docord_base = ws->w_dbase.as<int64_t>(); P.doc_tok = ws->w_doctok.as<int32_t>(); P.counters = ws->w_counters.as<int32_t>();
    P.giant_q = ws->w_gq.as<int64_t>(); P.giant_cap = total / kArenaPiece + 1; P.giant_cnt = ws->w_gcnt.as<int32_t>();
    P.giant_count = reinterpret_cast<unsigned long long*>(cb + offsetof(CounterBlock, heavy_count));
    P.giant_ticket = reinterpret_cast<unsigned long long*>(cb + offsetof(CounterBlock, giant_ticket));
    P.heavy_flag = ws->w_heavyq.as<uint8_t>(); P.nsub = (total + kSub - 1) / kSub;
    P.pool = ws->w_pool.as<int32_t>(); P.pool_head = reinterpret_cast<unsigned long long*>(cb + offsetof(CounterBlock, pool_head)); P.pool_cap = (int64_t)(ws->w_pool.cap / 4);
    return P;
}

#ifdef TKZ_DEVPROF
unsigned long long* g_devprof = nullptr;   // development builds only (make DEVPROF=1, env TKZ_DEV_ABLATE bit 4)
tkz_status devprof_arm(tkz::EncodeParams* P, hipStream_t stream) {
    { const char* ab = getenv("TKZ_DEV_ABLATE"); P->ablate = ab ? atoi(ab) : 0; }
    if (P->ablate & 16) {
        if (!g_devprof) { HIP_TRY(hipMalloc((void**)&g_devprof, 64 * 8)); }
        HIP_TRY(hipMemsetAsync(g_devprof, 0, 64 * 8, stream));
    }
    P->devprof = g_devprof;
    return TKZ_OK;
}
tkz_status devprof_report() {
    if (!g_devprof || !getenv("TKZ_DEV_ABLATE") || !(atoi(getenv("TKZ_DEV_ABLATE")) & 16)) return TKZ_OK;
    unsigned long long h[64];
    HIP_TRY(hipMemcpy(h, g_devprof, sizeof h, hipMemcpyDeviceToHost));
    const double w = h[0] ? (double)h[0] : 1.0;
    fprintf(stderr, "[tkz devprof] k_probe waves %llu  clock ticks/wave: total %.0f  load+compact %.0f  short batches %.0f  mid batches %.0f | mid pieces/wave %.1f pieces/wave %.1f\n",
            h[0], h[1] / w, h[2] / w, h[3] / w, h[4] / w, h[5] / w, h[6] / w);
    if (h[51]) fprintf(stderr, "[tkz devprof] k_probe lane-cycle table, per sub-tile: load+compact %.0f ticks (64 lanes) | 13+-byte pre-pass %.0f ticks, %.1f pieces in %.2f passes of 64 (lane use %.3f) | main loop: first bucket %.0f ticks at lane use %.3f (%.2f batches of 64, %.1f pieces), second bucket %.0f ticks for %.1f lanes (%.3f of the lanes of the iterations that run it: %.2f of %.2f iterations), records and lists %.0f ticks at lane use %.3f\n",
                       h[2] / w, h[4] / w, h[5] / w, (double)((h[5] + 63 * h[0]) / 64) / w, h[5] ? (double)h[5] / (64.0 * (double)((h[5] + 63 * h[0]) / 64)) : 0.0,
                       h[48] / w, (double)h[52] / (64.0 * (double)h[51]), h[51] / w, h[52] / w, h[49] / w, h[53] / w, h[54] ? (double)h[53] / (128.0 * (double)h[54]) : 0.0, h[54] / w, (double)((h[51] + 1) / 2) / w,
                       h[50] / w, (double)h[52] / (64.0 * (double)h[51]));
    if (h[8]) fprintf(stderr, "[tkz devprof] k_giant_merge pieces %llu  clock ticks/piece: rounds in global memory %.0f  the tail %.0f | bytes/piece %.0f tokens/piece %.0f | slowest piece %llu ticks | global rounds/piece %.2f | parts/piece when the tail took over %.0f\n",
                      h[8], (double)h[9] / h[8], (double)h[10] / h[8], (double)h[11] / h[8], (double)h[12] / h[8], h[13], (double)h[14] / h[8], (double)h[7] / h[8]);
    if (h[8]) fprintf(stderr, "[tkz devprof] slowest giant piece: %llu bytes -> %llu tokens, global rounds %llu (%llu ticks), bytes first/middle/last %02llx %02llx %02llx\n",
                      h[24], h[27], h[25], h[28], h[29] & 255, (h[29] >> 8) & 255, (h[29] >> 16) & 255);
    if (h[32]) fprintf(stderr, "[tkz devprof] k_merge_long waves %llu units %llu  ticks/wave %.0f | of all ticks: sort %.3f batch formation %.3f bytes %.3f first level %.3f merges %.3f emission %.3f | fast batches %llu lanes/batch %.1f steps/batch %.1f merges/lane %.2f lane use in the merge loop %.3f ticks/step %.0f\n",
                       h[32], h[44], (double)h[33] / h[32], (double)h[34] / h[33], (double)h[35] / h[33], (double)h[36] / h[33], (double)h[37] / h[33], (double)h[38] / h[33], (double)h[39] / h[33],
                       h[40], (double)h[41] / (h[40] ? h[40] : 1), (double)h[42] / (h[40] ? h[40] : 1), (double)h[43] / (h[41] ? h[41] : 1), (double)h[43] / (64.0 * (h[42] ? h[42] : 1)), (double)h[38] / (h[42] ? h[42] : 1));
    if (h[16]) fprintf(stderr, "[tkz devprof] tail: batches %llu merges %llu (%.2f a batch) proposals/batch %.1f | rounds for chains of equal pairs %llu | ticks/batch %.0f | longest tail: %llu batches, %llu ticks\n",
                       h[16], h[17], (double)h[17] / h[16], (double)h[18] / h[16], h[19], (double)h[22] / h[16], h[20], h[23]);
    return TKZ_OK;
}
#else
tkz_status devprof_arm(tkz::EncodeParams*, hipStream_t) { return TKZ_OK; }
tkz_status devprof_report() { return TKZ_OK; }
#endif

// the tiles of the longest stream a packed call of `total` bytes can produce (a token a byte at most, and the framing)
int64_t pack_tiles(int64_t total, int64_t n_docs, const PackCall& k) { return (total + k.frame() * n_docs + tkz::kPackTile - 1) / tkz::kPackTile; }

// A packed call on a batch without bytes: with framing ids its stream is not empty (T = f * n_docs), and the stage runs over offsets that are all 0.
tkz_status pack_empty(tkz_encoder* e, Workspace* ws, const BatchCall& c, int64_t* totals3) {
    using namespace tkz;
    const PackCall& k = *c.packed;
    const int64_t n_docs = c.n_docs;
    totals3[0] = totals3[1] = totals3[2] = 0;
    const Launch L{c.stream, nullptr, ws};
    HIP_TRY(ws->w_counts3.ensure(32, &ws->bytes_allocated));
    if (k.frame() * n_docs == 0) {
        launch_counts3(L, n_docs, 0, nullptr, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3);
        HIP_TRY(hipMemsetAsync(c.d_out_offs, 0, (size_t)(n_docs + 1) * sizeof(int64_t), c.stream));
        if (k.d_seg_starts) HIP_TRY(hipMemsetAsync(k.d_seg_starts, 0, sizeof(int64_t), c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        return TKZ_OK;
    }
    HIP_TRY(ws->pk_tot.ensure(64, &ws->bytes_allocated));
    HIP_TRY(hipMemsetAsync(ws->pk_tot.p, 0, 64, c.stream));
    HIP_TRY(hipMemsetAsync(ws->pk_offs.p, 0, (size_t)(n_docs + 1) * sizeof(int64_t), c.stream));
    int64_t* const tot = ws->pk_tot.as<int64_t>();
    const PackParams K{nullptr, 0, ws->pk_offs.as<int64_t>(), n_docs, tot + 3, k.bos_id, k.eos_id, k.pad_id, k.row_len,
                       c.d_out, c.out_cap, c.d_out_offs, k.d_pos, k.d_seg_starts, k.seg_cap,
                       ws->pk_cnt.as<int32_t>(), pack_tiles(0, n_docs, k), ws->pk_base.as<int64_t>(), ws->pk_bsum.as<int64_t>(), tot, reinterpret_cast<const int32_t*>(tot + 4)};
    launch_pack(L, K);
    launch_counts3(L, n_docs, 0, tot, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3);
    HIP_TRY(hipMemcpyAsync(totals3, tot, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    HIP_TRY(hipGetLastError());
    return TKZ_OK;
}

// the stage of a padded call over the uncut ids and offsets (the workspace's); blk: the counter block (its first word: the error bits), totals: its {total, W, n_cut}
tkz::PadParams pad_params(Workspace* ws, const BatchCall& c, const int64_t* grand, int64_t* totals, const int32_t* blk) {
    const PadCall& k = *c.padded;
    int32_t* const part = ws->pd_part.as<int32_t>();
    return tkz::PadParams{ws->pd_ids.as<int32_t>(), c.total, ws->pd_offs.as<int64_t>(), c.n_docs, grand, k.bos_id, k.eos_id, k.pad_id, k.max_len, k.cut_side, k.pad_side,
                          k.pad_multiple, c.d_out, c.out_cap, k.d_mask, k.d_pos, k.d_lens, c.d_out_offs, ws->pd_src.as<int64_t>(), part,
                          reinterpret_cast<int64_t*>(part + tkz::kPadGridMax), 0, totals, blk};
}

// the stage of a bucketed call: the padded stage's arguments and the workspace of the sort and the table (bucketed_on_device sizes it)
tkz::BktParams bkt_params(Workspace* ws, const BatchCall& c, const int64_t* grand, int64_t* totals, const int32_t* blk) {
    const BktCall& k = *c.bucketed;
    const int64_t n = std::max<int64_t>(c.n_docs, 1), nt = tkz::bkt_sort_tiles(c.n_docs);
    return tkz::BktParams{pad_params(ws, c, grand, totals, blk), k.bucket_rows, k.buckets(c.n_docs), k.order, 0, k.d_order, k.d_rank, k.d_bucket_offs, k.d_bucket_widths,
                          ws->bk_keys.as<uint32_t>(), ws->bk_idx.as<int64_t>(), ws->bk_keys.as<uint32_t>() + n, ws->bk_idx.as<int64_t>() + n, ws->bk_hist.as<int32_t>(),
                          ws->bk_base.as<int64_t>(), ws->bk_bsum.as<int64_t>(), ws->bk_base.as<int64_t>() + 256 * nt, ws->bk_cnt.as<int64_t>(), ws->bk_boffs.as<int64_t>(),
                          reinterpret_cast<int32_t*>(ws->bk_keys.as<uint32_t>() + 2 * n), ws->bk_idx.as<int64_t>() + 2 * n};
}

// the stage of a budgeted call: the bucketed stage's arguments (the sort's workspace; its table arrays hold min(n_docs, bucket_cap) buckets) and the workspace of the
// runs and the table (budgeted_on_device sizes it).  n_buckets_out: where the device stores n_buckets
tkz::TbkParams tbk_params(Workspace* ws, const BatchCall& c, const int64_t* grand, int64_t* totals, const int32_t* blk, int64_t* n_buckets_out) {
    const TbkCall& k = *c.budgeted;
    const int64_t tc = k.table_cap(c.n_docs), rc = tkz::tbk_run_cap(c.n_docs, c.padded->max_len, c.padded->pad_multiple), ng = tkz::tbk_mark_groups(c.n_docs);
    int64_t* const runs = ws->tb_runs.as<int64_t>();           // (five int64 arrays, then the two int32 ones)
    int64_t* const fig = ws->tb_fig.as<int64_t>();
    return tkz::TbkParams{bkt_params(ws, c, grand, totals, blk), k.token_budget, k.bucket_cap, tc, rc, k.d_bucket_rows, n_buckets_out,
                          reinterpret_cast<int32_t*>(ws->tb_marks.as<int64_t>() + ng), ws->tb_marks.as<int64_t>(), fig + 3,
                          runs, reinterpret_cast<int32_t*>(runs + 6 * rc), runs + rc, runs + 2 * rc, runs + 3 * rc, runs + 4 * rc, reinterpret_cast<int32_t*>(runs + 6 * rc) + rc,
                          runs + 5 * rc, fig, ws->tb_rows.as<int64_t>(), reinterpret_cast<int32_t*>(ws->tb_rows.as<int64_t>() + tc + 1)};
}

// A padded call on a batch without bytes: every document is its framing alone (all of them empty: W = 0 without framing), and the stage runs over offsets that
// are all 0.  Without documents there is nothing but the offset to clear.  A bucketed call likewise (its first bucket offset is cleared as well), and a budgeted
// one (its first bucket row too; n_buckets is the fourth figure: totals3 has four entries then).
tkz_status pad_empty(tkz_encoder* e, Workspace* ws, const BatchCall& c, int64_t* totals3) {
    using namespace tkz;
    const int64_t n_docs = c.n_docs;
    totals3[0] = totals3[1] = totals3[2] = 0;
    const Launch L{c.stream, nullptr, ws};
    HIP_TRY(ws->w_counts3.ensure(32, &ws->bytes_allocated));
    if (n_docs == 0) {
        launch_counts3(L, 0, 0, nullptr, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3);
        if (c.d_out_offs) HIP_TRY(hipMemsetAsync(c.d_out_offs, 0, sizeof(int64_t), c.stream));
        if (c.bucketed) HIP_TRY(hipMemsetAsync(c.bucketed->d_bucket_offs, 0, sizeof(int64_t), c.stream));
        if (c.budgeted) { HIP_TRY(hipMemsetAsync(c.budgeted->d_bucket_rows, 0, sizeof(int64_t), c.stream)); totals3[3] = 0; }
        HIP_TRY(hipStreamSynchronize(c.stream));
        return TKZ_OK;
    }
    HIP_TRY(ws->pd_tot.ensure(64, &ws->bytes_allocated));
    HIP_TRY(hipMemsetAsync(ws->pd_tot.p, 0, 64, c.stream));
    HIP_TRY(hipMemsetAsync(ws->pd_offs.p, 0, (size_t)(n_docs + 1) * sizeof(int64_t), c.stream));
    int64_t* const tot = ws->pd_tot.as<int64_t>();
    if (c.budgeted) launch_budgeted(L, tbk_params(ws, c, tot + 3, tot, reinterpret_cast<const int32_t*>(tot + 4), tot + 5));
    else if (c.bucketed) launch_bucketed(L, bkt_params(ws, c, tot + 3, tot, reinterpret_cast<const int32_t*>(tot + 4)));
    else launch_pad(L, pad_params(ws, c, tot + 3, tot, reinterpret_cast<const int32_t*>(tot + 4)));
    launch_counts3(L, n_docs, 0, tot, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3);
    HIP_TRY(hipMemcpyAsync(totals3, tot, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
    if (c.budgeted) HIP_TRY(hipMemcpyAsync(totals3 + 3, tot + 5, sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    HIP_TRY(hipGetLastError());
    return TKZ_OK;
}

// the stage of a pair call over the uncut ids and offsets (the workspace's); blk and totals as pad_params
tkz::PairParams pair_params(Workspace* ws, const BatchCall& c, const int64_t* grand, int64_t* totals, const int32_t* blk) {
    const PairCall& k = *c.pairs;
    const int64_t np = c.n_docs / 2;
    int32_t* const part = ws->pr_part.as<int32_t>();
    return tkz::PairParams{ws->pr_ids.as<int32_t>(), c.total, ws->pr_offs.as<int64_t>(), np, grand, k.bos_id, k.sep_id, k.sep_count, k.eos_id, k.pad_id, k.max_len,
                           k.strategy, k.cut_side, k.pad_side, k.pad_multiple, c.d_out, c.out_cap, k.d_mask, k.d_types, k.d_pos, k.d_lens, k.d_kept, c.d_out_offs,
                           ws->pr_src.as<int64_t>(), part, reinterpret_cast<int64_t*>(part + tkz::kPairGridMax), 0, totals, blk};
}

// A pair call on a batch without bytes, as pad_empty: every row is its framing alone (W = 0 without framing), and the stage runs over offsets that are all 0.
// Without documents there is nothing but the offset to clear.
tkz_status pair_empty(tkz_encoder* e, Workspace* ws, const BatchCall& c, int64_t* totals3) {
    using namespace tkz;
    const int64_t n_docs = c.n_docs;
    totals3[0] = totals3[1] = totals3[2] = 0;
    const Launch L{c.stream, nullptr, ws};
    HIP_TRY(ws->w_counts3.ensure(32, &ws->bytes_allocated));
    if (n_docs == 0) {
        launch_counts3(L, 0, 0, nullptr, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3);
        if (c.d_out_offs) HIP_TRY(hipMemsetAsync(c.d_out_offs, 0, sizeof(int64_t), c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        return TKZ_OK;
    }
    HIP_TRY(ws->pr_tot.ensure(64, &ws->bytes_allocated));
    HIP_TRY(hipMemsetAsync(ws->pr_tot.p, 0, 64, c.stream));
    HIP_TRY(hipMemsetAsync(ws->pr_offs.p, 0, (size_t)(n_docs + 1) * sizeof(int64_t), c.stream));
    int64_t* const tot = ws->pr_tot.as<int64_t>();
    launch_pairs(L, pair_params(ws, c, tot + 3, tot, reinterpret_cast<const int32_t*>(tot + 4)));
    launch_counts3(L, n_docs, 0, tot, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3);
    HIP_TRY(hipMemcpyAsync(totals3, tot, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    HIP_TRY(hipGetLastError());
    return TKZ_OK;
}

// One attempt on the stream: the zero region and the text (k_ingest), the document marks and the pre-tokenizer (or, on a re-run, the counters and the
// sub-tile flags only: it starts behind the pre-tokenizer), the counts of the marks and pieces and their scan, the piece index, then the sizing probe
// (nsample >= 0) or the whole launch sequence, and the counter block back to the host.
tkz_status enqueue_attempt(tkz_encoder* e, Workspace* ws, const tkz::Launch& L, const TkzTables& T, const BatchCall& c, bool marks_reused, int64_t nsample,
                           bool* pieces_over) {
    using namespace tkz;
    const hipStream_t stream = L.stream;
    const uint8_t* const d_bytes = c.d_bytes;
    const int64_t* const d_offs = c.d_offs;
    const int64_t n_docs = c.n_docs, total = c.total;
    PiecesOut* const po = c.pieces;
    const int64_t nwords = total / 64 + 1, ntiles = (total + kSub - 1) / kSub;
    int32_t* counters = ws->w_counters.as<int32_t>();
    char* cb = ws->w_counters.as<char>();
    uint64_t* docbits = ws->w_docbits.as<uint64_t>();
    uint64_t* startbits = ws->w_startbits.as<uint64_t>();
    const SpecialCall* const special = c.literals();
    int32_t* const has_empty = reinterpret_cast<int32_t*>(cb + offsetof(CounterBlock, has_empty));
    if (marks_reused) {      // (the counters and the sub-tile flags only; has_empty stays what the first attempt's k_docmark made it)
        HIP_TRY(hipMemsetAsync(ws->w_zero.p, 0, kCountersRerun, stream));
        if (!c.bitmap_only()) HIP_TRY(hipMemsetAsync(ws->w_heavyq.p, 0, (size_t)(ws->w_zero.as<char>() + ws->zero_bytes - ws->w_heavyq.as<char>()), stream));
    } else {
        if (c.ingest) launch_ingest(L, c.ingest->h_bytes, total, const_cast<uint8_t*>(d_bytes), c.ingest->h_offs, n_docs + 1, const_cast<int64_t*>(d_offs), ws->w_zero.p, (int64_t)ws->zero_bytes);
        // counters, document-start bits, sub-tile flags.  (A chunk of a host batch clears them with a kernel of its own, not a fill command: the runtime's fill is
        //  a blit kernel that queued behind its D2H blit of the chunk before -- the 16 MB call's second chunk started when the first one's download ended.)
        else if (ws->zero_bytes <= (size_t(8) << 20)) launch_ingest(L, nullptr, 0, nullptr, nullptr, 0, nullptr, ws->w_zero.p, (int64_t)ws->zero_bytes);
        else HIP_TRY(hipMemsetAsync(ws->w_zero.p, 0, ws->zero_bytes, stream));
        launch_docmark(L, d_offs, n_docs, total, docbits, counters, has_empty);
        // the special entries: the pre-tokenizer splits between SEGMENT marks (the documents cut at the literals taken), from a bitmap or -- the scanners that take
        // offsets: the sequential one, o200k's last resort -- from the segments' offsets
        const uint64_t* isobits = docbits;
        const int64_t* iso_offs = d_offs;
        int64_t n_iso = n_docs;
        if (special) {
            for (DevBuf* b : {&ws->w_candbits, &ws->w_segbits, &ws->w_specbits, &ws->w_endbits}) HIP_TRY(b->ensure((size_t)(nwords + 8) * 8, &ws->bytes_allocated));
            launch_lit_scan(L, d_bytes, total, docbits, nwords, e->LIT, special->allowed, ws->w_candbits.as<uint64_t>(), ws->w_segbits.as<uint64_t>(),
                            ws->w_specbits.as<uint64_t>(), ws->w_endbits.as<uint64_t>(), reinterpret_cast<unsigned long long*>(cb + offsetof(CounterBlock, n_literals)), c.d_repl);
            isobits = ws->w_segbits.as<uint64_t>();
            if (e->pretok_seq || e->pattern == TKZ_PATTERN_O200K || e->pattern == TKZ_PATTERN_O200K_DOTNET) {
                // (how many segments there are is known on the device only: one wait, as the piece-granular entry has it)
                int64_t* nseg = reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, ndocstarts));
                launch_doccount2(L, isobits, isobits, nwords, total, ntiles, ws->w_dcount.as<int32_t>(), ws->w_pcount.as<int32_t>());
                launch_scan2(L, ntiles, ws->w_bsum.as<int64_t>(), ws->w_dcount.as<int32_t>(), ws->w_dbase.as<int64_t>(), nseg, 1, nullptr, nullptr, nullptr, 1, -1);
                HIP_TRY(hipMemcpyAsync(&ws->h_counters->ndocstarts, nseg, 8, hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
                ws->n_seg = ws->h_counters->ndocstarts;
                HIP_TRY(ws->w_segoffs.ensure((size_t)(ws->n_seg + 2) * 8, &ws->bytes_allocated));
                launch_seg_offsets(L, isobits, nwords, total, ntiles, ws->w_dbase.as<int64_t>(), ws->n_seg, ws->w_segoffs.as<int64_t>());
                iso_offs = ws->w_segoffs.as<int64_t>();
                n_iso = ws->n_seg;
            }
        }
        if (!c.pretokenizes()) {
            HIP_TRY(hipMemcpyAsync(startbits, docbits, (size_t)nwords * 8, hipMemcpyDeviceToDevice, stream));
        } else if (e->pretok_seq) {
            HIP_TRY(hipMemcpyAsync(startbits, isobits, (size_t)nwords * 8, hipMemcpyDeviceToDevice, stream));
            launch_pretok_seq(L, e->pattern, d_bytes, iso_offs, n_iso, total, startbits, T.bmp_class, counters);
        } else {
            HIP_TRY(ws->w_xq.ensure((size_t)(nwords / kRowsPerWave + 4) * 16, &ws->bytes_allocated));     // two queues (launch_pretok_rows)
            launch_pretok_rows(L, e->pattern, d_bytes, iso_offs, n_iso, total, isobits, startbits, nwords, T.bmp_class, counters,
                               ws->w_xq.as<int64_t>(), reinterpret_cast<unsigned long long*>(cb + offsetof(CounterBlock, xcount)));
        }
        if (c.pretokenizes() && e->case_equiv && e->pattern == TKZ_PATTERN_CL100K) launch_case_equiv_fix(L, d_bytes, total, isobits, startbits);
        // (every taken literal ONE piece: the starts the pre-tokenizer found inside it go)
        if (special) launch_lit_fix(L, startbits, isobits, ws->w_specbits.as<uint64_t>(), ws->w_endbits.as<uint64_t>(), nwords);
    }
    if (c.bitmap_only()) {
        HIP_TRY(hipMemcpyAsync(c.d_bitmap, startbits, (size_t)nwords * 8, hipMemcpyDeviceToDevice, stream));
    } else {
        EncodeParams P = bind_params(ws, d_bytes, d_offs, n_docs, total);
        // (a batch of at most 16 MB waits for the slowest wavefront of every kernel, not for throughput: TKZ_OPT_LATENCY_BYTES, launch_encode.  Handing its
        //  pieces of 33..128 bytes to k_merge_coop as well was tried: 115 us in that kernel for what the lanes do in 6 -- a wavefront takes ~30 us a piece)
        P.lane_piece = kLanePiece;
        P.latency = total <= e->latency_bytes ? 1 : 0;
        // (... and in a small batch, whose three merge stages run as ONE launch -- k_merge_latency --, or beside one another: the token counts are summed with atomics)
        P.tc_atomic = (L.side || P.latency) ? 1 : 0;
        if (L.side && nsample < 0) ++ws->forked_batches;
        P.coop_cap = total / P.lane_piece + 64;
        P.coop_q = ws->w_coopq.as<uint64_t>();
        P.coop_count = reinterpret_cast<unsigned long long*>(cb + offsetof(CounterBlock, coop_count));
        P.coop_ticket = reinterpret_cast<unsigned long long*>(cb + offsetof(CounterBlock, coop_ticket));
        P.lq_cnt = ws->w_lqcnt.as<int32_t>(); P.lq_base = ws->w_lqbase.as<int64_t>(); P.lq = ws->w_lq.as<uint64_t>(); P.lq_cap = total / (kShortMax + 1) + 64;
        P.lq_total = reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, lq_total)); P.lq_bsum = ws->w_bsum.as<int64_t>();
        P.miss_sums = reinterpret_cast<unsigned long long*>(cb + offsetof(CounterBlock, miss_short));
        P.stats = e->piece_stats ? e->t_stats.as<unsigned long long>() : nullptr;
        // (statistics: an attempt that has to be run again -- lists or records to grow -- must not be counted twice: the block as it was before
        //  this attempt waits behind it and is put back on a retry)
        if (P.stats) HIP_TRY(hipMemcpyAsync(e->t_stats.as<char>() + 64, P.stats, 64, hipMemcpyDeviceToDevice, stream));
        P.place128 = ws->place128 ? 1 : 0;
        P.promo = T.promo; P.pextra = T.promo ? ws->w_pextra.as<int32_t>() : nullptr;
        if (ws->learning) {
            P.long_log = e->t_long_log.as<uint32_t>(); P.long_log_cap = (int32_t)kLongLogCap; P.long_log_sparse = T.memo_hits_sparse ? 1 : 0;
            P.long_log_count = reinterpret_cast<unsigned long long*>(e->t_long_log.as<char>() + (size_t)kLongLogCap * kLongLogDwords * 4);   // (the encoder's: it runs on through the batches of a window)
        }
        if (special) { P.specbits = ws->w_specbits.as<uint64_t>(); P.lit_meta = e->LIT.meta; P.lit_blob = e->LIT.blob; P.n_lit = e->LIT.n; P.lit_repl = c.d_repl; }
        TKZ_TRY(devprof_arm(&P, stream));
        int64_t* ndocstarts = reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, ndocstarts));
        int64_t* npieces = reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, npieces));
        int64_t* grand = reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, grand));
        // piece granularity: the piece-start bitmap takes the place of the document bitmap from here on, so that the encode
        // kernels record the token position of every PIECE start and k_docoffs yields the token range of every piece
        const uint64_t* markbits = po ? startbits : docbits;
        P.docbits = markbits;
        // the marks (document starts; at piece granularity the piece starts) and the piece starts of every sub-tile, counted in ONE pass over
        // the two bitmaps and scanned by ONE launch (the piece counts rounded up to whole record lines: where a sub-tile's records live in `prank`)
        launch_doccount2(L, markbits, startbits, nwords, total, ntiles, ws->w_dcount.as<int32_t>(), ws->w_pcount.as<int32_t>());
        launch_scan2(L, ntiles, ws->w_bsum.as<int64_t>(), ws->w_dcount.as<int32_t>(), ws->w_dbase.as<int64_t>(), ndocstarts, 1,
                     ws->w_pcount.as<int32_t>(), ws->w_pbase.as<int64_t>(), npieces, kRecordLine, -1);
        if (po) {
            HIP_TRY(hipMemcpyAsync(&ws->h_counters->ndocstarts, ndocstarts, 8, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            po->n_pieces = ws->h_counters->ndocstarts;                  // piece starts below `total` (a document start is one)
            // piece arrays too small: the launch sequence still runs to its end (without the piece arrays), so that the caller
            // learns BOTH required sizes from this one call (tkz.h: *n_pieces and *needed_ids on TKZ_E_CAPACITY)
            *pieces_over = po->n_pieces > po->piece_cap;
            if (c.piece_granular()) {                                   // (the workspace's piece arrays: sized for the pieces there are, not for one per byte)
                for (DevBuf* b : {&ws->p_boffs, &ws->p_toffs}) HIP_TRY(b->ensure((size_t)(po->n_pieces + 1) * 8, &ws->bytes_allocated));
                po->piece_boffs = ws->p_boffs.as<int64_t>(); po->piece_toffs = ws->p_toffs.as<int64_t>();
            }
            if (!*pieces_over) launch_piece_index(L, startbits, nwords, total, ntiles, ws->w_dbase.as<int64_t>(), po->n_pieces, po->piece_boffs, d_offs, n_docs, po->doc_piece);
        }
        if (nsample >= 0) {
            launch_probe_sample(L, T, P, nsample);
        } else {
            launch_encode(L, T, P, ntiles);
            if (P.stats) launch_miss_stats(L, P, ntiles);
            launch_scan2(L, ntiles, ws->w_bsum.as<int64_t>(), P.tile_count, ws->w_tbase.as<int64_t>(), grand, 1, nullptr, nullptr, nullptr, 1, K_SCAN);
            // (a trim call's untrimmed ids stay in the workspace: the caller's buffer holds the kept ones only)
            // (a count call: the token position of every mark and no ids)
            if (c.count_only) launch_tokcount(L, P, ws->w_tbase.as<int64_t>(), ws->w_dcount.as<int32_t>(), ntiles);
            // (a packed call that frames its documents: the unframed ids stay in the workspace too -- every one of them moves)
            else if (c.packed && c.packed->frame()) launch_place(L, P, ws->w_tbase.as<int64_t>(), ntiles, ws->pk_ids.as<int32_t>(), total);
            // (a padded call: the uncut ids likewise -- the rows are gathered from them)
            else if (c.padded) launch_place(L, P, ws->w_tbase.as<int64_t>(), ntiles, ws->pd_ids.as<int32_t>(), total);
            // (a pair call: the same -- the rows are gathered from the two texts' ids)
            else if (c.pairs) launch_place(L, P, ws->w_tbase.as<int64_t>(), ntiles, ws->pr_ids.as<int32_t>(), total);
            else launch_place(L, P, ws->w_tbase.as<int64_t>(), ntiles, c.trim ? ws->t_ids.as<int32_t>() : c.d_out, c.trim ? total : c.out_cap);
            if (po) {
                if (!*pieces_over) launch_docoffs(L, po->piece_boffs, po->n_pieces, total, ws->w_tbase.as<int64_t>(), markbits, P.docord_base, P.doc_tok, grand, po->piece_toffs, has_empty);
                const int64_t* produced = grand;
                if (c.trim) {
                    int64_t* const keep = ws->t_keep.as<int64_t>();
                    int64_t* const kept = reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, kept_total));
                    const TrimParams R{d_bytes, d_offs, n_docs, total, po->doc_piece, po->piece_boffs, po->piece_toffs, c.trim->side, c.trim->max_tokens, c.trim->d_max,
                                       keep, keep + n_docs, keep + 2 * n_docs, ws->t_bsum.as<int64_t>(), c.trim->d_cut_bytes, c.trim->d_cut_units, counters};
                    launch_trim(L, R, ws->t_ids.as<int32_t>(), total, c.d_out, c.out_cap, c.d_out_offs, kept);
                    produced = kept;
                }
                if (c.spans && !*pieces_over) {                         // (the position of every token, and the document offsets from the piece arrays)
                    HIP_TRY(hipMemsetAsync(ws->sp_intbits.p, 0, (size_t)nwords * 8, stream));
                    int32_t* const cnt = ws->sp_cnt.as<int32_t>();
                    int64_t* const base = ws->sp_base.as<int64_t>();
                    const SpanParams S{d_bytes, total, d_offs, n_docs, startbits, docbits, ws->sp_intbits.as<uint64_t>(), nwords, ntiles,
                                       po->doc_piece, po->piece_boffs, po->piece_toffs, po->n_pieces, c.d_out, c.out_cap, grand,
                                       cnt, cnt + ntiles, base, base + ntiles, base + 2 * ntiles, ws->w_bsum.as<int64_t>(),
                                       c.d_out_offs, c.spans->d_tok_bytes, c.spans->d_tok_units, counters};
                    launch_tokspans(L, S, e->D);
                }
                if (c.chunks && !*pieces_over) {                        // (the chunk table, and the document offsets from the piece arrays)
                    const ChunkCall& k = *c.chunks;
                    int64_t* const ubase = ws->ck_ubase.as<int64_t>();
                    const int64_t nspan = (total + kChunkUnitSpan - 1) / kChunkUnitSpan;
                    const ChunkParams C{d_bytes, total, d_offs, n_docs, po->doc_piece, po->piece_boffs, po->piece_toffs, c.d_out, c.out_cap, grand, k.max_tokens,
                                        ws->ck_cnt.as<int64_t>(), ws->ck_bsum.as<int64_t>(), ws->ck_list.as<int64_t>(),
                                        reinterpret_cast<unsigned long long*>(cb + offsetof(CounterBlock, chunk_long)),
                                        nspan, ws->ck_ucnt.as<int32_t>(), ubase, ubase + nspan + 2, ubase + nspan,
                                        c.d_out_offs, k.d_doc_chunk_offs, k.d_chunk_tokens, k.d_chunk_bytes, k.d_chunk_units, k.chunk_cap,
                                        reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, n_chunks)), counters};
                    if (k.overlap >= 0) launch_chunks_overlap(L, ChunkOvParams{C, k.overlap, k.d_chunk_ends, k.d_chunk_end_bytes, k.d_chunk_end_units}, e->D);
                    else launch_chunks(L, C, e->D);
                }
                launch_counts3(L, n_docs, total, produced, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3);
            } else if (c.packed) {                                      // (the unframed offsets, then the rows; the counts blocks receive T)
                const PackCall& k = *c.packed;
                const bool framed = k.frame() > 0;
                int64_t* const totals = reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, pack_total));
                int64_t* const unframed = framed ? ws->pk_offs.as<int64_t>() : c.d_out_offs;
                launch_docoffs(L, d_offs, n_docs, total, ws->w_tbase.as<int64_t>(), docbits, P.docord_base, P.doc_tok, grand, unframed, has_empty);
                const PackParams K{framed ? ws->pk_ids.as<int32_t>() : c.d_out, framed ? total : c.out_cap, unframed, n_docs, grand, k.bos_id, k.eos_id, k.pad_id, k.row_len,
                                   c.d_out, c.out_cap, c.d_out_offs, k.d_pos, k.d_seg_starts, k.seg_cap,
                                   ws->pk_cnt.as<int32_t>(), pack_tiles(total, n_docs, k), ws->pk_base.as<int64_t>(), ws->pk_bsum.as<int64_t>(), totals, counters};
                launch_pack(L, K);
                launch_counts3(L, n_docs, total, totals, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3);
            } else if (c.padded) {                                      // (the uncut offsets, then the rows; the counts blocks receive the uncut total)
                launch_docoffs(L, d_offs, n_docs, total, ws->w_tbase.as<int64_t>(), docbits, P.docord_base, P.doc_tok, grand, ws->pd_offs.as<int64_t>(), has_empty);
                if (c.budgeted) launch_budgeted(L, tbk_params(ws, c, grand, reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, pad_total)), counters,
                                                              reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, pad_buckets))));
                else if (c.bucketed) launch_bucketed(L, bkt_params(ws, c, grand, reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, pad_total)), counters));
                else launch_pad(L, pad_params(ws, c, grand, reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, pad_total)), counters));
                launch_counts3(L, n_docs, total, grand, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3);
            } else if (c.pairs) {                                       // (the uncut offsets, then the rows of the pairs; the counts blocks receive the uncut total)
                launch_docoffs(L, d_offs, n_docs, total, ws->w_tbase.as<int64_t>(), docbits, P.docord_base, P.doc_tok, grand, ws->pr_offs.as<int64_t>(), has_empty);
                launch_pairs(L, pair_params(ws, c, grand, reinterpret_cast<int64_t*>(cb + offsetof(CounterBlock, pad_total)), counters));
                launch_counts3(L, n_docs, total, grand, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3);
            } else      // (the batch's {n_docs, n_bytes, n_tokens} blocks by the same launch)
                launch_docoffs(L, d_offs, n_docs, total, ws->w_tbase.as<int64_t>(), docbits, P.docord_base, P.doc_tok, grand, c.d_out_offs,
                               has_empty, n_docs, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3);
        }
    }
    HIP_TRY(hipMemcpyAsync(ws->h_counters, counters, sizeof(CounterBlock), hipMemcpyDeviceToHost, stream));
    return TKZ_OK;
}

// The counter block of an attempt that has run: a failure status for input that is wrong or a buffer that cannot grow; TKZ_OK with *retry when a buffer
// was grown (or, after the sizing attempt, sized) and the batch runs again; TKZ_OK alone when the batch is done.
tkz_status check_counters(tkz_encoder* e, Workspace* ws, const BatchCall& call, int attempt, int64_t nsample, bool* retry) {
    using namespace tkz;
    const CounterBlock& c = *ws->h_counters;
    const int64_t total = call.total;
    const bool bitmap_only = call.bitmap_only();
    const int64_t ntiles = (total + kSub - 1) / kSub;
    int64_t* acc = &ws->bytes_allocated;
    const int32_t err = c.err;
    *retry = false;
    if (err & kErrOffsets) return fail(TKZ_E_ARG, "document offsets must start at 0, be non-decreasing and end at the byte count");
    if (err & kErrUtf8) return fail(TKZ_E_INVALID_UTF8, "input is not well-formed UTF-8 (or a document boundary falls inside a character)");
    if (err & kErrTooLong) return fail(TKZ_E_UNSUPPORTED, "a single piece longer than 2^30 bytes");
    if (err & kErrSpanDoc) return fail(TKZ_E_UNSUPPORTED, "token spans: a document of 2^31 bytes or more");
    // (what is wrong from here on is the size of a buffer)
    if (!bitmap_only) ws->sized = true;
    if (!bitmap_only && nsample < 0 && total > e->latency_bytes) {      // (the next batch's form of the long pieces' kernels: side_streams)
        ws->last_coop = (int64_t)c.coop_count;
        ws->last_lq_total = c.lq_total;
    }
    // k_place's form for THIS batch from the sample (it is otherwise chosen from the batch before: a fresh encoder's first miss-heavy batch ran
    // k_place<64> with most sub-tiles on its general path, 11.7 ms against 7)
    if (nsample >= 0 && (int64_t)c.over64 * 5 > nsample) { ws->place128 = true; ws->low_place = 0; }
    const bool last = attempt >= 4;
    if (err & kErrPool) {
        if (last) return fail(TKZ_E_OUT_OF_MEMORY, "long-piece scratch exhausted");
        // scratch for the giant pieces was too small.  pool_head keeps counting past the capacity, so it holds the exact need
        // (6 int32 per byte of every giant piece of the batch): size the pool for that -- not for the whole batch -- and rerun
        const size_t need = (size_t)c.pool_head * 4 + 4096;
        if (ws->w_pool.ensure(need, acc) != hipSuccess)
            return fail(TKZ_E_OUT_OF_MEMORY, "scratch for the pieces longer than 1024 bytes: " + std::to_string(need) + " bytes could not be allocated");
    } else if (err & kErrMissCap) {
        if (last) return fail(TKZ_E_DEVICE, "miss list overflow");
        // a sub-tile missed more pieces than its list holds (text where nearly every piece misses the vocabulary): the longest list
        // any sub-tile needed is known now -- longer lists for this workspace from here on, and the batch again
        int32_t want = kMissCapMin;
        while (want < c.mneed && want < kMissCapMax) want *= 2;
        if (want <= ws->mcap) return fail(TKZ_E_DEVICE, "miss list overflow");
        if (ws->w_mlist.ensure((size_t)ntiles * (size_t)want * 4, acc) != hipSuccess || ws->w_mquad.ensure((size_t)ntiles * (size_t)want * 16, acc) != hipSuccess)
            return fail(TKZ_E_OUT_OF_MEMORY, "miss lists: " + std::to_string((size_t)ntiles * (size_t)want * 20) + " bytes could not be allocated");
        ws->mcap = want;
    } else if (err & kErrCapacity) {          // more pieces than the record buffer was sized for: the exact count is known now
        if (last) return fail(TKZ_E_DEVICE, "piece record buffer overflow");
        const size_t need = ((size_t)c.npieces + 4096) * 4;
        if (ws->w_prank.ensure(need, acc) != hipSuccess)
            return fail(TKZ_E_OUT_OF_MEMORY, "piece records: " + std::to_string(need) + " bytes could not be allocated");
    } else if (nsample >= 0) {                // (the sample fitted the lists as they are; the records are counted exactly by the scan)
        const size_t need = ((size_t)c.npieces + 4096) * 4;
        if (need > ws->w_prank.cap && ws->w_prank.ensure(need, acc) != hipSuccess)
            return fail(TKZ_E_OUT_OF_MEMORY, "piece records: " + std::to_string(need) + " bytes could not be allocated");
    } else {
        if (err & kErrKeyNotFound) return fail(TKZ_E_KEY_NOT_FOUND, "a byte of the input is not in the vocabulary (KeyNotFoundException in the reference)");
        if (err & kErrSpanSum) return fail(TKZ_E_DEVICE, "token spans: the key lengths of a piece's ids do not add up to the piece");
        if (err & kErrChunkSum) return fail(TKZ_E_DEVICE, "chunks: the key lengths of an item's ids do not lead to a position inside the item");
        if (!bitmap_only && e->piece_stats) {
            std::lock_guard<std::mutex> lock(e->mu);
            ++e->stat_batches; e->stat_giants += (int64_t)c.heavy_count;
        }
        return TKZ_OK;
    }
    // the statistics block as it was before this attempt (enqueue_attempt): the batch is counted once
    if (e->piece_stats && e->t_stats.p && !bitmap_only) HIP_TRY(hipMemcpyAsync(e->t_stats.p, e->t_stats.as<char>() + 64, 64, hipMemcpyDeviceToDevice, call.stream));
    *retry = true;
    return TKZ_OK;
}

// Growing is immediate, shrinking waits for kLowBatches consecutive batches that would have done with less (the round-4 advisor: a
// workspace that alternates miss-heavy and ordinary batches -- or the 48 MB chunks of one host call that does -- must not overflow,
// re-run, free and re-allocate on every other batch).
void settle_workspace(Workspace* ws, int64_t ntiles) {
    using namespace tkz;
    constexpr int kLowBatches = 3;
    const bool heavy = (int64_t)ws->h_counters->over64 * 5 > ntiles;      // (more than a fifth of the sub-tiles: the next batches' k_place)
    if (heavy) { ws->place128 = true; ws->low_place = 0; }
    else if (ws->place128 && ++ws->low_place >= kLowBatches) { ws->place128 = false; ws->low_place = 0; }
    if (ws->mcap <= kMissCapMin) return;
    // lists that were grown for an earlier batch (text where nearly every piece misses) and that the last kLowBatches batches filled to
    // less than half: half as long from here on (one step at a time), and the buffers given back when they are far larger than such
    // batches need (the lists are ntiles * mcap * 20 bytes: 1.25 B per input byte at 64 entries, 20 B at 1024)
    int32_t want = kMissCapMin;
    while (want < ws->h_counters->mhigh) want *= 2;
    if (want >= ws->mcap) ws->low_lists = 0;
    else if (++ws->low_lists >= kLowBatches) {
        ws->low_lists = 0;
        ws->mcap = std::max(want, ws->mcap / 2);
        if (ws->w_mquad.cap > (size_t)ntiles * (size_t)ws->mcap * 16 * 4) {
            ws->bytes_allocated -= (int64_t)(ws->w_mquad.cap + ws->w_mlist.cap);
            ws->w_mquad.release(); ws->w_mlist.release();
        }
    }
}

// a learning window's promotion, or the drop of the promotions for a re-learn: on a thread of its own behind the batch (after_batch)
void promote_or_drop(tkz_encoder* e, bool promote) {
    DeviceScope scope;
    const bool dev = scope.enter(e->device) == hipSuccess;
    if (promote) {
        int64_t added = 0;
        size_t held;
        { std::lock_guard<std::mutex> lock(e->mu); held = e->promo_items.size(); }
        if (dev) (void)promote_from_memo(e, true, true, &added);   // (a failure leaves the tables as they were)
        std::lock_guard<std::mutex> lock(e->mu);
        e->policy.promotion_installed(added, held);
    } else {
        if (dev) (void)drop_promotions(e, true);
        std::lock_guard<std::mutex> lock(e->mu);
        e->policy.promotions_dropped();
    }
}

// The batch is done: if it completes a learning window, the hottest entries are promoted now (the copy of the memo back to the host and the
// rebuilt key tables cost tens of milliseconds: on a thread, behind the batch); else the share of pieces that missed the key tables is
// compared with what it was after the last promotion (AdaptPolicy::batch_ended decides, under the lock; the thread starts outside it)
void after_batch(tkz_encoder* e, Workspace* ws, int64_t total) {
    const CounterBlock& c = *ws->h_counters;
    tkz::AdaptPolicy::After what;
    {
        std::lock_guard<std::mutex> lock(e->mu);
        what = e->policy.batch_ended(total, (double)(c.miss_short + c.miss_long), (double)c.npieces, ws->learning, e->promo_items.size(), ws->tables_gen);
        ws->learning = false;
    }
    const bool promote = what == tkz::AdaptPolicy::After::Promote;
    if (!promote && what != tkz::AdaptPolicy::After::Relearn) return;
    // (the workspace is this call's no longer once it returns; the counters, the log and the memo are the encoder's, and no other batch writes the
    //  first two while the policy's learning slot is taken)
    join_promotion(e);                 // (the previous one ended before this batch could be armed: this only reaps the thread)
    bool started = false;
    {
        std::lock_guard<std::mutex> jl(e->promo_join_mu);
        try { e->promo_thread = std::thread(promote_or_drop, e, promote); started = true; } catch (...) {}      // (no thread to be had: built here, as before round 5)
    }
    if (!started) { const std::string keep_msg = g_err; promote_or_drop(e, promote); g_err = keep_msg; }
}

// The batch on the device.
// phase: kCallWhole -- enqueue, wait, evaluate (and again if a buffer had to grow); kCallBegin -- enqueue the first attempt and
// return; kCallEnd -- wait for that attempt, evaluate, and carry on as kCallWhole does (tkz_encode_batch_device_begin / _end)
tkz_status encode_device(tkz_encoder* e, Workspace* ws, const BatchCall& c, int phase, int64_t* total_tokens) {
    using namespace tkz;
    const int64_t n_docs = c.n_docs, total = c.total;
    const hipStream_t stream = c.stream;
    if (n_docs < 0 || total < 0 || c.out_cap < 0) return fail(TKZ_E_ARG, "negative size");
    if (c.count_only && !c.plain_encode()) return fail(TKZ_E_ARG, "a count call is an encode call");
    if (total_tokens) *total_tokens = 0;
    if (n_docs == 0 && total != 0) return fail(TKZ_E_ARG, "bytes without documents");
    // the outcome of a packed call: the three figures, and the capacity they are held against (tkz.h)
    const auto packed_done = [&](const int64_t* totals3) {
        const PackCall& k = *c.packed;
        if (total_tokens) *total_tokens = totals3[0];
        if (k.n_rows) *k.n_rows = totals3[1];
        if (k.n_segs) *k.n_segs = totals3[2];
        if (totals3[1] * k.row_len > c.out_cap) return fail(TKZ_E_CAPACITY, "output capacity too small for the rows");
        if (k.d_seg_starts && totals3[2] > k.seg_cap) return fail(TKZ_E_CAPACITY, "segment table capacity too small");
        return TKZ_OK;
    };
    if (total == 0 && c.packed) {
        int64_t totals3[3];
        TKZ_TRY(pack_empty(e, ws, c, totals3));
        return packed_done(totals3);
    }
    // the outcome of a padded call likewise: the uncut total, the width and the cut documents; n_docs * W against the capacity
    const auto padded_done = [&](const int64_t* totals3) {
        const PadCall& k = *c.padded;
        if (total_tokens) *total_tokens = totals3[0];
        if (k.width) *k.width = totals3[1];
        if (k.n_cut) *k.n_cut = totals3[2];
        if (c.budgeted) {                                         // (pad_buckets lies behind the three: n_buckets; both capacities, all four figures)
            if (c.budgeted->n_buckets) *c.budgeted->n_buckets = totals3[3];
            if (totals3[1] > c.out_cap) return fail(TKZ_E_CAPACITY, "output capacity too small for the rows");
            return totals3[3] > c.budgeted->bucket_cap ? fail(TKZ_E_CAPACITY, "bucket table capacity too small") : TKZ_OK;
        }
        if (c.bucketed) return totals3[1] > c.out_cap ? fail(TKZ_E_CAPACITY, "output capacity too small for the rows") : TKZ_OK;      // (totals3[1]: P, the positions)
        if (totals3[1] > 0 && n_docs > c.out_cap / totals3[1]) return fail(TKZ_E_CAPACITY, "output capacity too small for the rows");
        return TKZ_OK;
    };
    if (total == 0 && c.padded) {
        int64_t totals3[4];
        TKZ_TRY(pad_empty(e, ws, c, totals3));
        return padded_done(totals3);
    }
    // the outcome of a pair call: the uncut total, the width and the cut pairs; n_pairs * W against the capacity
    const auto pairs_done = [&](const int64_t* totals3) {
        const PairCall& k = *c.pairs;
        if (total_tokens) *total_tokens = totals3[0];
        if (k.width) *k.width = totals3[1];
        if (k.n_cut) *k.n_cut = totals3[2];
        if (totals3[1] > 0 && n_docs / 2 > c.out_cap / totals3[1]) return fail(TKZ_E_CAPACITY, "output capacity too small for the rows");
        return TKZ_OK;
    };
    if (total == 0 && c.pairs) {
        int64_t totals3[3];
        TKZ_TRY(pair_empty(e, ws, c, totals3));
        return pairs_done(totals3);
    }
    if (total == 0) {
        if (phase != kCallEnd) {                                  // (kCallEnd: enqueued when it began)
            HIP_TRY(ws->w_counts3.ensure(32, &ws->bytes_allocated));
            { Launch L0{stream, nullptr, ws}; launch_counts3(L0, n_docs, 0, nullptr, e->t_counts3.as<int64_t>(), ws->w_counts3.as<int64_t>(), c.d_counts3); }
            if (c.d_out_offs) HIP_TRY(hipMemsetAsync(c.d_out_offs, 0, (size_t)(n_docs + 1) * sizeof(int64_t), stream));
            if (c.chunks) {                                       // (no chunks: both offset arrays cleared, and the token total behind the last chunk)
                HIP_TRY(hipMemsetAsync(c.chunks->d_doc_chunk_offs, 0, (size_t)(n_docs + 1) * sizeof(int64_t), stream));
                if (c.chunks->overlap < 0) HIP_TRY(hipMemsetAsync(c.chunks->d_chunk_tokens, 0, sizeof(int64_t), stream));      // (the overlap entries' table has no entry behind the last chunk)
            }
            if (c.trim && n_docs > 0) for (int64_t* cut : {c.trim->d_cut_bytes, c.trim->d_cut_units}) if (cut) HIP_TRY(hipMemsetAsync(cut, 0, (size_t)n_docs * sizeof(int64_t), stream));
            if (c.d_bitmap) { const uint64_t one = 1; HIP_TRY(hipMemcpyAsync(c.d_bitmap, &one, 8, hipMemcpyHostToDevice, stream)); }
            if (phase == kCallBegin) return TKZ_OK;               // (_begin returns without waiting)
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return TKZ_OK;
    }
    const int64_t ntiles = (total + kSub - 1) / kSub;       // sub-tiles: one wavefront each
    SlowCallLog slow_log(total);
    TKZ_TRY(prepare_workspace(ws, total, n_docs, c.kind));
    if (!ws->h_counters) HIP_TRY(hipHostMalloc((void**)&ws->h_counters, sizeof(CounterBlock), 0));

    // a learning batch that ends any other way than with its promotion gives the encoder's one learning slot back
    struct LearnGuard {
        tkz_encoder* e; Workspace* ws; bool keep = false;
        ~LearnGuard() { if (!keep && ws->learning) { ws->learning = false; std::lock_guard<std::mutex> lock(e->mu); e->policy.learning_abandoned(); } }
    } learn_guard{e, ws};
    // An attempt that has to be run again (lists, records or scratch to grow) leaves the document marks and the piece-start bitmap as they are: the
    // next one starts behind the pre-tokenizer.
    bool marks_ready = false;
    for (int attempt = 0; attempt < 5; ++attempt) {
        slow_log.attempts = attempt + 1;
        bool pieces_over = false;
        const int64_t nsample = attempt == 0 && phase == kCallWhole && !ws->sized && c.plain_encode() ? sizing_sample(ntiles) : -1;
        const bool marks_reused = marks_ready;
        Launch L{stream, e->profiling ? prof_hook : nullptr, ws};
        side_streams(e, ws, total, &L);
        if (!(phase == kCallEnd && attempt == 0)) {              // (kCallEnd: the first attempt is in flight already)
            TkzTables T;
            TKZ_TRY(arm_learning(e, ws, c, attempt == 0, &T));
            TKZ_TRY(enqueue_attempt(e, ws, L, T, c, marks_reused, nsample, &pieces_over));
        }
        if (phase == kCallBegin) { learn_guard.keep = true; return TKZ_OK; }
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipGetLastError());
        if (e->profiling) prof_collect(ws);
        if (!c.bitmap_only()) TKZ_TRY(devprof_report());
        if (!marks_reused) { e->last_xcount = (int64_t)ws->h_counters->xcount; e->last_xcount2 = (int64_t)ws->h_counters->xcount2; ws->spec_taken = (int64_t)ws->h_counters->n_literals; }
        bool retry = false;
        TKZ_TRY(check_counters(e, ws, c, attempt, nsample, &retry));
        marks_ready = true;
        if (retry) continue;
        if (c.bitmap_only()) return TKZ_OK;
        settle_workspace(ws, ntiles);
        if (c.pretokenizes()) after_batch(e, ws, total);
        if (c.literals()) e->spec_literals += ws->spec_taken;
        if (c.packed) return packed_done(&ws->h_counters->pack_total);
        if (c.padded) return padded_done(&ws->h_counters->pad_total);
        if (c.pairs) return pairs_done(&ws->h_counters->pad_total);
        const int64_t produced = c.trim ? ws->h_counters->kept_total : ws->h_counters->grand;      // (a trim call's capacity counts the kept ids)
        if (total_tokens) *total_tokens = produced;
        if (c.chunks && c.chunks->n_chunks) *c.chunks->n_chunks = ws->h_counters->n_chunks;      // (both required sizes from one call)
        if (pieces_over) return fail(TKZ_E_CAPACITY, "piece arrays too small");
        if (!c.count_only && produced > c.out_cap) return fail(TKZ_E_CAPACITY, "output capacity too small");      // (a count call stores no ids)
        if (c.chunks && ws->h_counters->n_chunks > c.chunks->chunk_cap) return fail(TKZ_E_CAPACITY, "chunk table capacity too small");
        return TKZ_OK;
    }
    return fail(TKZ_E_DEVICE, "unreachable");
}

// ---- the single-launch path (k_small) --------------------------------------------------------------------------------------------------
// ITokenizer.Encode(text) on a prompt is microseconds in the reference (TikTokenizer.cs:178-207); the batch path above costs ~25 kernel
// launches, four copy commands and two synchronisations whatever the size: ~160 us for 64 bytes.  A batch of at most kSmallMaxBytes bytes
// in at most kSmallMaxDocs documents of at most kSmallMaxDoc bytes each goes through ONE launch instead: the caller's bytes and offsets
// are memcpy'd into a page-locked block, k_small (one workgroup, all phases) reads them from there and writes ids, offsets and status
// back into it, one stream synchronisation, memcpy out.  Returns TKZ_OK with *handled = false when the kernel hands the batch back (a
// piece of more than 1024 bytes, an error to be diagnosed, lists or buffers to be grown): the caller then takes the batch path.
constexpr size_t kSmallOffBytes = 0, kSmallOffOffs = tkz::kSmallMaxBytes + 64, kSmallOffIds = kSmallOffOffs + (tkz::kSmallMaxDocs + 1) * 8,
                 kSmallOffOut = kSmallOffIds + tkz::kSmallMaxBytes * 4, kSmallOffRes = kSmallOffOut + (tkz::kSmallMaxDocs + 1) * 8, kSmallOffRepl = kSmallOffRes + 256,
                 kSmallBlock = kSmallOffRepl + tkz::kSmallMaxBytes / 8 + 8;     // (the replaced-byte bitmap of a special call on text transcoded from UTF-16: total / 64 + 1 words)
bool small_eligible(const tkz_encoder* e, const int64_t* offs, int64_t n_docs, int64_t total) {
    if (!e->small_ok || e->profiling || e->pretok_seq || (e->case_equiv && e->pattern == TKZ_PATTERN_CL100K) || total <= 0 || total > tkz::kSmallMaxBytes || n_docs < 1 || n_docs > tkz::kSmallMaxDocs) return false;
    const bool o200k = e->pattern == TKZ_PATTERN_O200K || e->pattern == TKZ_PATTERN_O200K_DOTNET;
    if (o200k && total > tkz::kSmallMaxBytesO200k) return false;
    if (o200k)                                    // (split by the sequential matcher there, one lane per document)
        for (int64_t d = 0; d < n_docs; ++d) { const int64_t len = offs[d + 1] - offs[d]; if (len < 0 || len > tkz::kSmallMaxDoc) return false; }
    return true;
}
tkz_status encode_small(tkz_encoder* e, Workspace* ws, const HostCall& c, bool* handled) {
    using namespace tkz;
    const int64_t n_docs = c.n_docs, total = c.total();
    *handled = false;
    // (a trim call: a token mark per possible piece, as the batch trim path has them)
    { const tkz_status ps = prepare_workspace(ws, total, n_docs, c.trim ? CallKind::Trim : CallKind::Encode); if (ps != TKZ_OK) return ps; }
    int64_t* acc = &ws->bytes_allocated;
    HIP_TRY(ws->s_bytes[0].ensure((size_t)kSmallMaxBytes + 64, acc));
    HIP_TRY(ws->s_offs[0].ensure((size_t)(kSmallMaxDocs + 1) * 8, acc));
    if (!ws->h_small) HIP_TRY(hipHostMalloc((void**)&ws->h_small, kSmallBlock, 0));
    if (!ws->st_small) HIP_TRY(hipStreamCreateWithFlags(&ws->st_small, hipStreamNonBlocking));
    uint8_t* H = ws->h_small;
    memcpy(H + kSmallOffBytes, c.bytes, (size_t)total);
    memcpy(H + kSmallOffOffs, c.offs, (size_t)(n_docs + 1) * 8);
    int64_t* h_res = reinterpret_cast<int64_t*>(H + kSmallOffRes);
    h_res[0] = -1; h_res[1] = 0; h_res[2] = 0; h_res[3] = 0;
    EncodeParams P = bind_params(ws, ws->s_bytes[0].as<uint8_t>(), ws->s_offs[0].as<int64_t>(), n_docs, total);
    P.lane_piece = kSmallLanePiece;
    SmallArgs A{};
    A.h_bytes = H + kSmallOffBytes; A.h_offs = reinterpret_cast<const int64_t*>(H + kSmallOffOffs);
    A.out = reinterpret_cast<int32_t*>(H + kSmallOffIds); A.out_cap = c.count_only ? (int64_t)kSmallMaxBytes : std::min<int64_t>(c.out_cap, kSmallMaxBytes); A.out_offs = reinterpret_cast<int64_t*>(H + kSmallOffOut);
    A.h_result = h_res;
    A.docbits = ws->w_docbits.as<uint64_t>(); A.startbits = ws->w_startbits.as<uint64_t>();
    A.pcount = ws->w_pcount.as<int32_t>(); A.pbase = ws->w_pbase.as<int64_t>(); A.docord_base = ws->w_dbase.as<int64_t>(); A.tile_base = ws->w_tbase.as<int64_t>();
    A.counter_words = (int32_t)(sizeof(CounterBlock) / 4);
    A.counts3[0] = e->t_counts3.as<int64_t>(); A.counts3[1] = ws->w_counts3.as<int64_t>();
    TkzTables T;
    { std::lock_guard<std::mutex> lock(e->mu); T = e->T; }
    P.promo = T.promo; P.pextra = T.promo ? ws->w_pextra.as<int32_t>() : nullptr;
    if (c.special) {       // the special form of the launch: the literal search of enqueue_attempt, inside it
        const int64_t nwords = total / 64 + 1;
        for (DevBuf* b : {&ws->w_candbits, &ws->w_segbits, &ws->w_specbits, &ws->w_endbits}) HIP_TRY(b->ensure((size_t)(nwords + 8) * 8, acc));
        A.lit = e->LIT; A.allowed = c.special->allowed;
        A.candbits = ws->w_candbits.as<uint64_t>(); A.segbits = ws->w_segbits.as<uint64_t>(); A.specbits = ws->w_specbits.as<uint64_t>(); A.endbits = ws->w_endbits.as<uint64_t>();
        A.n_taken = reinterpret_cast<unsigned long long*>(ws->w_counters.as<char>() + offsetof(CounterBlock, n_literals));
        if (c.repl) { memcpy(H + kSmallOffRepl, c.repl, (size_t)nwords * 8); A.repl = reinterpret_cast<const uint64_t*>(H + kSmallOffRepl); }
        P.specbits = A.specbits; P.lit_meta = e->LIT.meta; P.lit_blob = e->LIT.blob; P.n_lit = e->LIT.n; P.lit_repl = A.repl;
        P.stats = e->piece_stats ? e->t_stats.as<unsigned long long>() : nullptr;
    }
    if (c.trim) {          // the trim form: the marks are the piece starts (enqueue_attempt's `markbits = startbits`); the untrimmed ids all fit the block
        P.docbits = ws->w_startbits.as<uint64_t>();
        A.out_cap = kSmallMaxBytes;
        A.trim = 1; A.trim_side = c.trim->side; A.trim_max = c.trim->max_tokens;
        h_res[20] = 0; h_res[21] = 0; h_res[22] = 0; h_res[23] = 0;
    }
    Launch L{ws->st_small, nullptr, ws};
    launch_small(L, T, P, A);
    HIP_TRY(hipStreamSynchronize(ws->st_small));
    HIP_TRY(hipGetLastError());
    ws->small_calls.fetch_add(1, std::memory_order_relaxed);
    { std::lock_guard<std::mutex> lock(e->mu); memcpy(ws->small_clocks, h_res + 4, sizeof ws->small_clocks); }
    if (h_res[0] != 0) { ws->small_fallbacks.fetch_add(1, std::memory_order_relaxed); return TKZ_OK; }          // (handled stays false)
    const int64_t first = c.trim ? h_res[20] : 0, tokens = c.trim ? h_res[21] : h_res[2];        // (a trim call: the kept ids are [first, first + tokens) of the block's)
    if (c.needed) *c.needed = tokens;
    *handled = true;
    if (c.special) e->spec_literals += h_res[3];
    if (c.count_only) {      // (the ids stay in the page-locked block, which holds them whatever their number)
        memcpy(c.out_offsets, H + kSmallOffOut, (size_t)(n_docs + 1) * 8);
        if (c.took_single) *c.took_single = true;
        return TKZ_OK;
    }
    if (tokens > c.out_cap) return fail(TKZ_E_CAPACITY, "output capacity too small");
    if (tokens) memcpy(c.out_ids, H + kSmallOffIds + (size_t)first * 4, (size_t)tokens * 4);
    if (c.trim) {
        c.out_offsets[0] = 0; c.out_offsets[1] = tokens;
        if (c.trim->cut_bytes) *c.trim->cut_bytes = h_res[22];
        if (c.trim->cut_units) *c.trim->cut_units = h_res[23];
    } else memcpy(c.out_offsets, H + kSmallOffOut, (size_t)(n_docs + 1) * 8);
    return TKZ_OK;
}

tkz_status check_encoder(tkz_encoder* e, DeviceScope& scope) {
    if (!e) return fail(TKZ_E_ARG, "null encoder");
    hipError_t r = scope.enter(e->device);
    if (r != hipSuccess) return fail(TKZ_E_NO_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(r));
    return TKZ_OK;
}

hipError_t ensure_streams(Workspace* ws) {
    hipError_t r = hipSuccess;
    if (!ws->st_compute) r = hipStreamCreate(&ws->st_compute);
    if (r == hipSuccess && !ws->st_in) r = hipStreamCreate(&ws->st_in);
    if (r == hipSuccess && !ws->st_out) r = hipStreamCreate(&ws->st_out);
    for (int q = 0; q < 2 && r == hipSuccess; ++q) if (!ws->ev_in[q]) r = hipEventCreate(&ws->ev_in[q]);
    for (int q = 0; q < 3 && r == hipSuccess; ++q) if (!ws->ev_out[q]) r = hipEventCreate(&ws->ev_out[q]);
    return r;
}

// Is p page-locked host memory the device can address (tkz_host_alloc, hipHostMalloc, a torch pinned tensor)?  *dev: its device-side address.
bool pinned_host(const void* p, void** dev) {
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }      // (pageable memory: an error by design)
    if (a.type != hipMemoryTypeHost) return false;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) != hipSuccess || !d) { (void)hipGetLastError(); return false; }
    *dev = d;
    return true;
}

// host buffers -> staging -> device path -> back, for documents given as UTF-8 bytes (`bytes`) or as UTF-16 code units (`units`: uploaded as they are,
// Encoding.UTF8.GetBytes -- TikTokenizer.cs:261 -- runs on the device; offsets in units then).
//  * at most 128 KiB of UTF-8: the single-launch kernel (encode_small);
//  * one chunk (plan_host_batch: an upload below 1.5 chunks) from ordinary buffers: encode_host_blocking.  From page-locked caller buffers the inputs are copied
//    asynchronously and -- up to 8 MB of text -- the ids and offsets are written by the kernels STRAIGHT into the caller's memory (k_place / k_docoffs store whole
//    lines over PCIe): no download commands, one synchronisation (HostPipeline, its one iteration);
//  * larger: document ranges of a chunk each, pipelined (HostPipeline::run) -- the upload of chunk k+2 (and, for UTF-16, its length pass), the launch sequences of
//    chunks k+1 and k+2 (enqueued ahead, on two workspaces) and the download of chunk k (page-locked results: on a copy engine of its own, tkz_sdma.h) run at the
//    same time.  512 MB of page-locked text: 22 -> 37 GB/s, 64 MB: 22 -> 29.5 (profiles/r06/host_batches_ab.txt); what bounds it now is the download of the ids at
//    the link's duplex rate.
const char* const kMsgEngineDownload = "a copy engine reported an error for a download";
constexpr int64_t kHostChunkMin = int64_t(8) << 20;      // a chunk is at least this large (smaller ones were measured through an environment knob: profiles/r06/host_batches_ab.txt)

// How a host batch travels: which of the caller's buffers are page-locked, the chunks it is cut into, where its results are written.  Host arithmetic only.
struct HostPlan {
    bool pin_in = false, pin_out = false;              // page-locked caller buffers (a single chunk then needs no staging for its results; the copies of every path are asynchronous)
    void *dv_in = nullptr, *dv_offs = nullptr, *dv_ids = nullptr, *dv_ooffs = nullptr;      // ... as the device addresses them
    int64_t unit = 1, up_bytes = 0, chunk_bytes = 0, nchunks = 1;
    std::vector<int64_t> cut;                          // chunk k = documents [cut[k], cut[k+1])
    bool blocking = false;                             // one chunk, ordinary (pageable) buffers: encode_host_blocking
    bool direct_out = false, ingest_in = false;        // one small chunk on page-locked buffers: the kernels write the caller's results / fetch the caller's text themselves
    int nout = 1;                                      // output staging sets in use
    int64_t max_units = 0, max_docs = 0;               // the largest chunk
};
HostPlan plan_host_batch(const HostCall& c) {
    HostPlan p;
    const bool u16 = c.u16();
    const int64_t* const offs = c.offs;
    const int64_t n_docs = c.n_docs, total = c.total();
    p.pin_in = pinned_host(u16 ? (const void*)c.units : (const void*)c.bytes, &p.dv_in) && pinned_host(offs, &p.dv_offs);
    p.pin_out = !c.bitmap && pinned_host(c.out_offsets, &p.dv_ooffs) && (c.out_cap == 0 || pinned_host(c.out_ids, &p.dv_ids));
    // (16 MB of upload a chunk.  Until round 6 a chunk's kernels were launched when the chunk before had drained, every chunk paid its launch sequence's
    //  floor of ~0.4 ms and 32 MB chunks were the optimum; with two launch sequences enqueued ahead and the downloads on a copy engine of their own the
    //  floor is hidden: profiles/r06/host_batches_ab.txt.  Pageable buffers keep 32 MB: the runtime stages their copies itself, synchronously, a cost per copy)
    // ($TKZ_HOST_CHUNK_BYTES: test knob, so that the CPU-emulated tests can exercise the pipeline on kilobytes)
    static const int64_t kChunkEnv = [] { const char* v = getenv("TKZ_HOST_CHUNK_BYTES"); const long long n = v ? atoll(v) : 0; return n > 0 ? (int64_t)n : (int64_t)0; }();
    const int64_t kChunkBytes = kChunkEnv ? kChunkEnv : (p.pin_in && p.pin_out ? int64_t(16) << 20 : int64_t(32) << 20);
    p.unit = u16 ? 2 : 1;
    p.up_bytes = total * p.unit;
    // (from 12 MB up a batch is two chunks at least, of 8 MB or more: the second chunk's upload runs beside the first one's kernels)
    p.chunk_bytes = std::min(kChunkBytes, std::max(std::min(kChunkBytes, kHostChunkMin), p.up_bytes / 2));
    p.nchunks = (!c.plain_encode() || 2 * p.up_bytes < 3 * p.chunk_bytes) ? 1 : std::min<int64_t>(1024, std::max<int64_t>(2, (p.up_bytes + p.chunk_bytes / 2) / p.chunk_bytes));
    // chunk boundaries on documents.  Offsets that are not monotone cannot be cut: the whole batch then goes as one chunk and the device reports them (k_docmark)
    std::vector<int64_t>& cut = p.cut;
    cut.assign((size_t)p.nchunks + 1, 0);
    cut[(size_t)p.nchunks] = n_docs;
    for (int64_t k = 1; k < p.nchunks; ++k) {
        const int64_t want = total / p.nchunks * k;
        cut[(size_t)k] = std::lower_bound(offs, offs + n_docs, want) - offs;
        if (cut[(size_t)k] < cut[(size_t)k - 1] || offs[cut[(size_t)k]] < offs[cut[(size_t)k - 1]]) { p.nchunks = 1; break; }
    }
    if (p.nchunks == 1) { cut.assign(2, 0); cut[1] = n_docs; }
    p.blocking = !u16 && p.nchunks == 1 && !(p.pin_in && p.pin_out && c.plain_encode() && total > 0);
    // the kernels write the caller's page-locked ids and offsets themselves -- up to 8 MB of text: beyond that a DMA download beats k_place's stores over PCIe
    // (measured, round 5: 16 MB 1.08 ms direct, 1.00 ms staged)
    p.direct_out = p.nchunks == 1 && p.pin_out && p.up_bytes <= (int64_t(8) << 20) * p.unit;
    // (... and no upload stream at all: the launch sequence starts with k_ingest, which fetches the text itself)
    p.ingest_in = p.direct_out && !u16 && p.pin_in && total > 0 && (reinterpret_cast<uintptr_t>(p.dv_in) & 15) == 0;
    p.nout = p.nchunks > 2 ? 3 : (int)p.nchunks;
    for (int64_t k = 0; k < p.nchunks; ++k) {
        p.max_units = std::max(p.max_units, offs[cut[(size_t)k + 1]] - offs[cut[(size_t)k]]);
        p.max_docs = std::max(p.max_docs, cut[(size_t)k + 1] - cut[(size_t)k]);
    }
    return p;
}

// ---- the steps a host entry is composed from: validate, stage in, (transcode / decode lengths, the device call,) fetch -------------------------------
// What is said of a host batch's documents: of a first offset that is not 0, of items without a buffer, of a negative total, of an empty batch with other offsets than 0
struct DocKind { const char* first; const char* no_data; const char* negative; const char* not_empty; };
const char* const kMsgDocFirst = "doc_offsets[0] must be 0";
const DocKind kByteDocs{kMsgDocFirst, "null buffer", "negative byte count", kMsgByteOffsets}, kUnitDocs{kMsgDocFirst, "null buffer", "negative unit count", kMsgUnitOffsets},
              kSizedDocs{kMsgDocFirst, "null buffer", "negative size", kMsgByteOffsets}, kIdDocs{"id_offsets[0] must be 0", "bad id count", "bad id count", nullptr};
// The caller's offsets before anything is read through them: n_docs, the array, items behind a positive total, a first offset of 0, a total that is not negative.
tkz_status check_host_docs(const int64_t* offs, int64_t n_docs, bool have_data, const DocKind& kind, int64_t* total) {
    if (n_docs < 0 || !offs) return fail(TKZ_E_ARG, "null buffer");
    if (n_docs > 0 && !have_data && offs[n_docs] > 0) return fail(TKZ_E_ARG, kind.no_data);
    if (offs[0] != 0) return fail(TKZ_E_ARG, kind.first);
    *total = offs[n_docs];
    if (*total < 0) return fail(TKZ_E_ARG, kind.negative);
    return TKZ_OK;
}
// ... and of a batch with a total of 0, which no kernel looks at: every offset is 0 -- and so is every offset of the result (out_offsets, or null)
tkz_status check_empty_docs(const int64_t* offs, int64_t n_docs, const DocKind& kind, int64_t* out_offsets) {
    for (int64_t d = 0; d < n_docs; ++d) if (offs[d] != 0) return fail(TKZ_E_ARG, kind.not_empty);
    if (out_offsets) std::fill_n(out_offsets, n_docs + 1, int64_t(0));
    return TKZ_OK;
}
// the caller's result buffers: offsets always, items when there is room for any (trim: a capacity below 0 is refused here as well)
tkz_status check_host_outputs(const void* out_items, int64_t out_cap, const void* out_offsets, const char* msg = "null output buffer", bool negative_cap_ok = true) {
    if (!out_offsets || (out_cap > 0 && !out_items) || (out_cap < 0 && !negative_cap_ok)) return fail(TKZ_E_ARG, msg);
    return TKZ_OK;
}

// Whole-batch staging, for the entries that run ONE device call on pageable buffers: blocking copies on the null stream into and out of staging set 0.
tkz_status stage_in(Workspace* ws, const uint8_t* bytes, int64_t total, const int64_t* offs, int64_t n_docs) {
    HIP_TRY(ws->s_bytes[0].ensure((size_t)total + 64, &ws->bytes_allocated));
    HIP_TRY(ws->s_offs[0].ensure((size_t)(n_docs + 1) * 8, &ws->bytes_allocated));
    if (total) HIP_TRY(hipMemcpy(ws->s_bytes[0].p, bytes, (size_t)total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ws->s_offs[0].p, offs, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    return TKZ_OK;
}
tkz_status stage_out(Workspace* ws, int64_t n_docs, int64_t cap, bool with_offsets = true, bool with_ids = true) {      // (with_ids false: a count call)
    if (with_ids) HIP_TRY(ws->s_out[0].ensure((size_t)std::max<int64_t>(cap, 1) * 4, &ws->bytes_allocated));
    if (with_offsets) HIP_TRY(ws->s_outoffs[0].ensure((size_t)(n_docs + 1) * 8, &ws->bytes_allocated));
    return TKZ_OK;
}
tkz_status fetch(Workspace* ws, int32_t* out_ids, int64_t tokens, int64_t* out_offsets, int64_t n_docs) {      // (out_offsets null: the ids only)
    if (tokens) HIP_TRY(hipMemcpy(out_ids, ws->s_out[0].p, (size_t)tokens * 4, hipMemcpyDeviceToHost));
    if (out_offsets) HIP_TRY(hipMemcpy(out_offsets, ws->s_outoffs[0].p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost));
    return TKZ_OK;
}
BatchCall staged_call(Workspace* ws, int64_t n_docs, int64_t total, int64_t cap) {      // the batch stage_in / stage_out left on the device
    return BatchCall{ws->s_bytes[0].as<uint8_t>(), ws->s_offs[0].as<int64_t>(), n_docs, total, ws->s_out[0].as<int32_t>(), cap, ws->s_outoffs[0].as<int64_t>(), nullptr};
}

// one chunk, ordinary (pageable) buffers: blocking copies either side of the launch sequence
tkz_status encode_host_blocking(tkz_encoder* e, Workspace* ws, const HostCall& c) {
    uint64_t* const bitmap = c.bitmap;
    const int64_t n_docs = c.n_docs, total = c.total();
    const int64_t cap = bitmap ? 0 : std::min<int64_t>(c.out_cap, total);   // tokens <= bytes: more capacity is never used
    TKZ_TRY(stage_in(ws, c.bytes, total, c.offs, n_docs));
    if (bitmap) HIP_TRY(ws->s_out[0].ensure((size_t)(total / 64 + 1) * 8, &ws->bytes_allocated));
    else TKZ_TRY(stage_out(ws, n_docs, cap, true, !c.count_only));
    int64_t tokens = 0;
    BatchCall dc = c.on_device(ws->s_bytes[0].as<uint8_t>(), ws->s_offs[0].as<int64_t>(), n_docs, total, c.count_only ? nullptr : ws->s_out[0].as<int32_t>(), cap, ws->s_outoffs[0].as<int64_t>(), nullptr);
    if (bitmap) dc.d_bitmap = ws->s_out[0].as<uint64_t>();
    const tkz_status st = encode_device(e, ws, dc, kCallWhole, &tokens);
    if (c.needed) *c.needed = tokens;
    if (st != TKZ_OK) return st;
    if (bitmap) {
        HIP_TRY(hipMemcpy(bitmap, ws->s_out[0].p, (size_t)(total / 64 + 1) * 8, hipMemcpyDeviceToHost));
        return TKZ_OK;
    }
    return fetch(ws, c.out_ids, c.count_only ? 0 : tokens, c.out_offsets, n_docs);
}

// Inside the pipeline a failed runtime call is RECORDED (HostPipeline::note), never returned from encode_host: the upload of a later chunk may still be reading the
// caller's text and the download of an earlier one writing the caller's ids, and the caller is free to release both the moment it sees the error; HostPipeline::drain
// always runs first.  The `return` leaves the member function the macro stands in, no more.
#define PIPELINE_TRY(expr) { const hipError_t e_ = (expr); if (e_ != hipSuccess) return this->note(fail(TKZ_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_))); }

// Chunks on three streams (a single chunk is the loop's one iteration).
// TWO chunks' launch sequences are enqueued ahead (round 6).  Until then a chunk's kernels were launched when the chunk before had drained -- the host
// needs its token count to place the download --, so the device idled for the ~25 launches of every chunk (tools/gpu_job_sdma.sh: 64 MB as 8 chunks took
// 1.5 ms longer than as 2, ~250 us a chunk, whatever the download did).  Now chunk k + 2 is begun (encode_device, kCallBegin: enqueue and return) the
// moment chunk k has ended (kCallEnd: wait, evaluate, retry if a list has to grow), on the workspace and the stream chunk k has just left: odd and even chunks
// alternate between two leased workspaces, two input staging sets and -- since the download of chunk k is only ISSUED when k has ended -- three output sets.
struct HostPipeline {
    // the call
    tkz_encoder* e; Workspace* ws; const HostPlan& p; const HostCall& c;
    const bool u16 = c.u16();
    const bool with_repl = u16 && c.special && c.special->fffd;      // the literal search must tell a lone surrogate's U+FFFD from a real one
    const int64_t* const offs = c.offs;
    int64_t* const acc = &ws->bytes_allocated;
    // its state
    std::unique_ptr<Lease> lease_b;
    Workspace* W[2] = {ws, ws};
    // what encode_device was given for the chunk in flight on W[q]: kCallEnd is handed the same.  (`ingest` stays set there.  It is read when the marks are not
    // reused only, and a chunk that is ended has its first attempt -- the one that makes the marks -- behind it.)
    BatchCall fl[2] = {};
    const IngestSrc ingest_src{static_cast<const uint8_t*>(p.dv_in), static_cast<const int64_t*>(p.dv_offs)};
    std::vector<int64_t> tok_base = std::vector<int64_t>((size_t)p.nchunks + 1, 0);
    bool over = false;                                       // out_cap exceeded: the remaining chunks are only counted
    bool sdma_out = false;                                   // downloads by copy engine (reserve_staging)
    bool sig_pending[3] = {false, false, false}, sigo_pending[3] = {false, false, false}, ev_pending[3] = {false, false, false};
    tkz_status first_err = TKZ_OK;
    std::string first_msg;

    tkz_status note(tkz_status s) { if (first_err == TKZ_OK) { first_err = s; first_msg = g_err; } return s; }
    // (the two workspaces forget each other before the second one's lease ends: the members are destroyed after this body)
    ~HostPipeline() { for (Workspace* w : W) { w->sibling = nullptr; w->chunk_in_flight = false; } }

    // streams, the second workspace, staging for the largest chunk, the copy engine's signals.  Nothing is in flight yet: a failure here is returned as it is
    tkz_status reserve_staging() {
        using namespace tkz;
        const int64_t nchunks = p.nchunks, max_units = p.max_units, max_docs = p.max_docs;
        HIP_TRY(ensure_streams(ws));
        if (nchunks > 1) {
            lease_b.reset(new Lease(e));
            W[1] = lease_b->ws;
            // this call's own: a learning window that needs the memo emptied may open while nothing is in flight on the sibling (arm_learning) -- chunk 0
            W[0]->sibling = W[1]; W[1]->sibling = W[0];
            if (!W[1]->st_compute) HIP_TRY(hipStreamCreate(&W[1]->st_compute));
        }
        for (int q = 0; q < (nchunks > 1 ? 2 : 1); ++q) {
            if (u16) {
                HIP_TRY(ws->u16[q].ensure(max_units, max_docs, acc, with_repl));
            } else {
                HIP_TRY(ws->s_bytes[q].ensure((size_t)max_units + 64, acc));
                HIP_TRY(ws->s_offs[q].ensure((size_t)(max_docs + 1) * 8, acc));
            }
        }
        if (!p.direct_out) for (int o = 0; o < p.nout; ++o) {
            if (!c.count_only) HIP_TRY(ws->s_out[o].ensure((size_t)std::max<int64_t>(std::min<int64_t>(c.out_cap, (u16 ? 3 : 1) * max_units), 1) * 4, acc));      // (a token is at least one byte, a code unit at most three)
            HIP_TRY(ws->s_outoffs[o].ensure((size_t)(max_docs + 1) * 8, acc));
        }
        // downloads by copy engine: page-locked results whose device-side address is their host address (hipHostMalloc, tkz_host_alloc, torch's pinned tensors --
        // not memory registered after the fact, which the HSA runtime knows under another address)
        if (ws->sdma_state == 0) {
            bool ok = sdma_available(e->device);
            for (int o = 0; o < 3 && ok; ++o) ok = sdma_signal_create(&ws->sig_out[o]) && sdma_signal_create(&ws->sig_outoffs[o]);
            ws->sdma_state = ok ? 1 : -1;
        }
        sdma_out = ws->sdma_state == 1 && !p.direct_out && p.pin_out && p.dv_ooffs == (void*)c.out_offsets && (c.out_cap == 0 || p.dv_ids == (void*)c.out_ids);
        return TKZ_OK;
    }
    // the input of chunk k, on its way to the device (stream st_in); for UTF-16 also its document marks, the UTF-8 length of every unit and their scan
    tkz_status stage_in(int64_t k) {
        using namespace tkz;
        const std::vector<int64_t>& cut = p.cut;
        const int q = (int)(k & 1);
        const int64_t d0 = cut[(size_t)k], d1 = cut[(size_t)k + 1], u0 = offs[d0], nu = offs[d1] - u0, nd = d1 - d0;
        Launch L{ws->st_in, nullptr, ws};
        if (u16) {
            U16Stage& U = ws->u16[q];
            if (nu) HIP_TRY(hipMemcpyAsync(U.units.p, c.units + u0, (size_t)nu * 2, hipMemcpyHostToDevice, ws->st_in));
            HIP_TRY(hipMemcpyAsync(U.offs.p, offs + d0, (size_t)(nd + 1) * 8, hipMemcpyHostToDevice, ws->st_in));
            if (u0) launch_rebase(L, U.offs.as<int64_t>(), nd + 1, u0);
            HIP_TRY(u16_measure(U, L, nu, nd));
        } else {
            if (nu) HIP_TRY(hipMemcpyAsync(ws->s_bytes[q].p, c.bytes + u0, (size_t)nu, hipMemcpyHostToDevice, ws->st_in));
            HIP_TRY(hipMemcpyAsync(ws->s_offs[q].p, offs + d0, (size_t)(nd + 1) * 8, hipMemcpyHostToDevice, ws->st_in));
            if (u0) launch_rebase(L, ws->s_offs[q].as<int64_t>(), nd + 1, u0);
        }
        HIP_TRY(hipEventRecord(ws->ev_in[q], ws->st_in));
        return TKZ_OK;
    }
    bool wait_engine(int o) {                // the copies of output set o that went by engine have arrived
        bool ok = true;
        if (sig_pending[o]) { sig_pending[o] = false; ok = tkz::sdma_signal_wait(ws->sig_out[o]) && ok; }
        if (sigo_pending[o]) { sigo_pending[o] = false; ok = tkz::sdma_signal_wait(ws->sig_outoffs[o]) && ok; }
        return ok;
    }
    // enqueue chunk k's launch sequence behind its upload (one chunk: run it whole -- phase kCallWhole)
    tkz_status begin_chunk(int64_t k, int phase, int64_t* tokens) {
        using namespace tkz;
        const std::vector<int64_t>& cut = p.cut;
        const int q = (int)(k & 1), o = (int)(k % p.nout);
        Workspace* w = W[q];
        const int64_t d0 = cut[(size_t)k], d1 = cut[(size_t)k + 1], nu = offs[d1] - offs[d0], nd = d1 - d0;
        const uint8_t* cb; const int64_t* co; int64_t cbytes;      // the chunk as UTF-8 on the device
        if (u16) {
            // the UTF-8 size of the chunk is known once its length pass is through (the host needs it: the launch shapes of the encode path)
            U16Stage& U = ws->u16[q];
            PIPELINE_TRY(hipEventSynchronize(ws->ev_in[q]));
            { const tkz_status us = u16_write(U, Launch{w->st_compute, nullptr, w}, nu, nd, with_repl, acc, &cbytes); if (us != TKZ_OK) return note(us); }
            cb = U.bytes.as<uint8_t>(); co = U.boffs.as<int64_t>();
        } else {
            if (!p.ingest_in) PIPELINE_TRY(hipStreamWaitEvent(w->st_compute, ws->ev_in[q], 0));
            cb = ws->s_bytes[q].as<uint8_t>(); co = ws->s_offs[q].as<int64_t>(); cbytes = nu;
        }
        // the download of chunk k - nout has left this chunk's output set
        if (!wait_engine(o)) return note(fail(TKZ_E_DEVICE, kMsgEngineDownload));
        if (ev_pending[o]) { ev_pending[o] = false; PIPELINE_TRY(hipStreamWaitEvent(w->st_compute, ws->ev_out[o], 0)); }
        int32_t* const dst_ids = c.count_only ? nullptr : p.direct_out ? static_cast<int32_t*>(p.dv_ids) : ws->s_out[o].as<int32_t>();      // (a count call: no ids anywhere)
        int64_t* const dst_offs = p.direct_out ? static_cast<int64_t*>(p.dv_ooffs) : ws->s_outoffs[o].as<int64_t>();
        // (how much of out_cap the chunks before leave is not known yet when a chunk is begun: the staging set holds a chunk's ids whatever their number, and the
        //  sum is checked when the chunk ends)
        fl[q] = c.on_device(cb, co, nd, cbytes, dst_ids, over ? 0 : std::min<int64_t>(c.out_cap, cbytes), dst_offs, w->st_compute);
        if (p.ingest_in) fl[q].ingest = &ingest_src;
        if (with_repl) fl[q].d_repl = ws->u16[q].repl.as<uint64_t>();
        // (in flight from the moment anything of it may be enqueued -- arm_learning of the OTHER workspace's next chunk asks -- until end_chunk has drained it)
        w->chunk_in_flight = phase == kCallBegin;
        return encode_device(e, w, fl[q], phase, tokens);
    }
    tkz_status end_chunk(int64_t k, int64_t* tokens) {          // (returns when the chunk's stream has drained)
        const tkz_status st = encode_device(e, W[k & 1], fl[k & 1], kCallEnd, tokens);
        W[k & 1]->chunk_in_flight = false;
        return st;
    }
    // (an engine that refuses a copy is not asked again: that copy and the rest of the call go through the runtime)
    bool by_engine(void* dst, const void* src, size_t nb, tkz::SdmaSignal sg, bool* pending) {
        using namespace tkz;
        if (!sdma_out) return false;
        sdma_signal_arm(sg, 1);
        if (sdma_copy_d2h(e->device, dst, src, nb, sg)) { *pending = true; ws->engine_downloads.fetch_add(1, std::memory_order_relaxed); return true; }
        sdma_signal_arm(sg, 0); sdma_out = false; ws->sdma_state = -1;
        return false;
    }
    // The download of chunk k.  The runtime's D2H copy of page-locked memory is a blit KERNEL and other kernels make no progress beside it (traced, round 5; a
    // small-grid download kernel of our own stalled their first stores until its PCIe writes had drained).  Page-locked results therefore leave on a COPY ENGINE
    // of their own, named through the HSA runtime (tkz_sdma.h; tools/sdma_probe.hip: 56 GB/s beside a store-heavy kernel, and beside the runtime's upload
    // when the engines differ).  The kernels of the chunk have completed (end_chunk returned), which is all such a copy waits for.
    tkz_status download(int64_t k, int64_t tokens) {
        const int o = (int)(k % p.nout);
        const int64_t d0 = p.cut[(size_t)k], nd = p.cut[(size_t)k + 1] - d0;
        // ONE writer for every entry of the caller's offsets: a chunk brings back the entry of each of its documents, nd of them, and not the one behind --
        // that is the next chunk's first (or out_offsets[n_docs]), and run() sets it from tok_base.  (Two chunks writing it relied on the later copy landing
        // last, which nothing orders once one goes by copy engine and the other through the runtime.)
        bool ids_sent = tokens == 0 || c.count_only, offs_sent = nd == 0;      // (a count call: only the offsets travel back; a chunk without documents: nothing does)
        const size_t nb_ids = (size_t)tokens * 4, nb_offs = (size_t)nd * 8;
        if (!ids_sent) ids_sent = by_engine(c.out_ids + tok_base[(size_t)k], ws->s_out[o].p, nb_ids, ws->sig_out[o], &sig_pending[o]);
        if (!offs_sent) offs_sent = by_engine(c.out_offsets + d0, ws->s_outoffs[o].p, nb_offs, ws->sig_outoffs[o], &sigo_pending[o]);
        if (!ids_sent || !offs_sent) {
            if (!ids_sent) PIPELINE_TRY(hipMemcpyAsync(c.out_ids + tok_base[(size_t)k], ws->s_out[o].p, nb_ids, hipMemcpyDeviceToHost, ws->st_out));
            if (!offs_sent) PIPELINE_TRY(hipMemcpyAsync(c.out_offsets + d0, ws->s_outoffs[o].p, nb_offs, hipMemcpyDeviceToHost, ws->st_out));
            PIPELINE_TRY(hipEventRecord(ws->ev_out[o], ws->st_out));
            ev_pending[o] = true;
        }
        return TKZ_OK;
    }
    bool finish(int64_t k, tkz_status cs, int64_t tokens) {      // chunk k has ended with status cs: its place in the output, its download; false: stop
        tok_base[(size_t)k + 1] = tok_base[(size_t)k] + tokens;
        if (cs == TKZ_E_CAPACITY || (cs == TKZ_OK && !c.count_only && tok_base[(size_t)k + 1] > c.out_cap)) { over = true; return true; }
        if (cs != TKZ_OK) { note(cs); return false; }
        if (!over && !p.direct_out && download(k, tokens) != TKZ_OK) return false;
        return true;
    }
    void drain() {                           // every copy of the call has left the caller's buffers
        (void)hipStreamSynchronize(ws->st_in);      // (an error of the runtime here is an error of the copies above: reported by them or by the next call)
        (void)hipStreamSynchronize(ws->st_out);
        for (int o = 0; o < 3; ++o)
            if (!wait_engine(o)) note(fail(TKZ_E_DEVICE, kMsgEngineDownload));
    }
    tkz_status run() {
        const int64_t nchunks = p.nchunks;
        int64_t begun = 0, ended = 0;            // chunks [ended, begun) are in flight
        HostTrace trace;
        if (nchunks == 1) {
            int64_t tokens = 0;
            const tkz_status ss = p.ingest_in ? TKZ_OK : stage_in(0);
            if (ss == TKZ_OK) { const tkz_status cs = begin_chunk(0, kCallWhole, &tokens); if (first_err == TKZ_OK) (void)finish(0, cs, tokens); }
            else note(ss);
        } else {
            // (upload 1 is issued BEHIND launch sequence 0, although that starts it ~130 us late: an upload stream's k_rebase kernel waits in a hardware queue for its copy, and
            //  the launch sequence of chunk 0 enqueued behind it -- the runtime maps its streams onto a few hardware queues -- waited with it: 16 MB 884 -> 1,040 us)
            for (int64_t k = 0; k < 2 && first_err == TKZ_OK; ++k) {
                { const tkz_status ss = stage_in(k); if (ss != TKZ_OK) { note(ss); break; } }
                const tkz_status bs = begin_chunk(k, kCallBegin, nullptr);
                if (bs != TKZ_OK) { note(bs); break; }
                ++begun;
                trace.stamp("begun", k);
            }
            for (int64_t k = 0; k < nchunks && first_err == TKZ_OK; ++k) {
                int64_t tokens = 0;
                const tkz_status cs = end_chunk(k, &tokens);
                ++ended;
                trace.stamp("ended", k);
                if (!finish(k, cs, tokens)) break;
                trace.stamp("download issued", k);
                if (k + 2 < nchunks) {         // (its input set and its workspace are chunk k's: free now)
                    tkz_status bs = stage_in(k + 2);
                    if (bs == TKZ_OK) bs = begin_chunk(k + 2, kCallBegin, nullptr);
                    if (bs != TKZ_OK) { note(bs); break; }
                    ++begun;
                    trace.stamp("begun", k + 2);
                }
            }
            // (a chunk that was begun is always ended: its workspace may hold the encoder's learning slot, and its kernels write the staging sets)
            for (; ended < begun; ++ended) { const std::string keep = g_err; int64_t t = 0; (void)end_chunk(ended, &t); g_err = keep; }
        }
        drain();
        if (nchunks > 1) { trace.stamp("downloads arrived", nchunks); trace.print(nchunks); }
        if (first_err != TKZ_OK) return fail(first_err, first_msg);
        if (c.needed) *c.needed = tok_base[(size_t)nchunks];
        if (over) return fail(TKZ_E_CAPACITY, "output capacity too small");
        // the offsets came back relative to their chunk: add the chunk's token base (chunk 0 needs nothing; the first entry of a later chunk came
        // back as 0 and gets that chunk's base -- the total of the chunks before; no chunk brought the entry behind its last document: download)
        for (int64_t k = 1; k < nchunks; ++k) {
            const int64_t tb = tok_base[(size_t)k];
            for (int64_t d = p.cut[(size_t)k]; d < p.cut[(size_t)k + 1]; ++d) c.out_offsets[d] += tb;
        }
        c.out_offsets[c.n_docs] = tok_base[(size_t)nchunks];
        return TKZ_OK;
    }
};
#undef PIPELINE_TRY

// validate -> the single-launch path -> plan -> one blocking chunk, or the pipeline
tkz_status encode_host(tkz_encoder* e, const HostCall& c) {
    DeviceScope scope;
    tkz_status st = check_encoder(e, scope);
    if (st != TKZ_OK) return st;
    const bool u16 = c.u16();
    const int64_t* const offs = c.offs;
    const int64_t n_docs = c.n_docs;
    int64_t total = 0;
    TKZ_TRY(check_host_docs(offs, n_docs, c.bytes || c.units, u16 ? kUnitDocs : kByteDocs, &total));
    if (c.needed) *c.needed = 0;
    if (u16 && total == 0) return check_empty_docs(offs, n_docs, kUnitDocs, c.out_offsets);
    if (c.count_only && total == 0) return check_empty_docs(offs, n_docs, kByteDocs, c.out_offsets);      // (an empty batch: zero offsets, nothing launched)
    Lease lease(e);
    Workspace* ws = lease.ws;
    // (the single-launch path first: at most 128 KiB, a fraction of a chunk -- and none of the planner's questions are asked of a 64-byte prompt)
    // (of the special calls only the single-text entries': a UTF-16 one brings the text as the host transcoded it)
    const HostCall* const sm = c.small_form ? c.small_form : u16 ? nullptr : &c;
    if (sm && sm->plain_encode() && (!sm->special || sm->single) && small_eligible(e, sm->offs, sm->n_docs, sm->total())) {
        bool handled = false;
        st = encode_small(e, ws, *sm, &handled);
        if (st != TKZ_OK || handled) return st;
    }
    const HostPlan plan = plan_host_batch(c);
    if (plan.blocking) return encode_host_blocking(e, ws, c);
    HostPipeline pipe{e, ws, plan, c};
    TKZ_TRY(pipe.reserve_staging());
    return pipe.run();
}

// tkz_encode_batch_utf8 and its special form; tkz_encode_pieces
tkz_status encode_host_batch(tkz_encoder* e, const HostCall& c) {
    TKZ_TRY(check_host_outputs(c.out_ids, c.out_cap, c.out_offsets));
    const tkz_status st = encode_host(e, c);
    if (st == TKZ_OK && c.special) ++e->spec_batches;
    return st;
}

// tkz_encode_batch_utf16 and its special form (sp null: the plain one)
tkz_status encode_host_batch_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const SpecialCall* sp,
                                   int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* needed, bool count_only = false) {
    HostCall c{nullptr, units, unit_offsets, n_docs, out_ids, out_cap, out_offsets, needed};
    c.utf16 = true; c.special = sp; c.count_only = count_only;
    return encode_host_batch(e, c);
}

// what the device entries check before they take a workspace
tkz_status check_device_call(tkz_encoder* e, DeviceScope& scope, const BatchCall& c) {
    TKZ_TRY(check_encoder(e, scope));
    if (!c.d_offs || !c.d_out_offs || (c.total > 0 && (!c.d_bytes || (!c.d_out && !c.count_only)))) return fail(TKZ_E_ARG, "null device buffer");
    if (reinterpret_cast<uintptr_t>(c.d_bytes) & 15) return fail(TKZ_E_ARG, "d_bytes must be 16-byte aligned");
    return TKZ_OK;
}

// tkz_encode_batch_device and its special form
tkz_status encode_device_batch(tkz_encoder* e, const BatchCall& c, int64_t* total_tokens) {
    DeviceScope scope;
    TKZ_TRY(check_device_call(e, scope, c));
    Lease lease(e);
    const tkz_status st = encode_device(e, lease.ws, c, kCallWhole, total_tokens);
    if (st == TKZ_OK && c.special) ++e->spec_batches;
    return st;
}

const char* const kRegexP1 = "'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+";
const char* const kRegexCl100k =
    "(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\\r\\n\\p{L}\\p{N}]?\\p{L}+|\\p{N}{1,3}| ?[^\\s\\p{L}\\p{N}]+[\\r\\n]*|\\s*[\\r\\n]+|\\s+(?!\\S)|\\s+";
#define TKZ_O2_SUFFIX "(?:'s|'S|'t|'T|'re|'RE|'Re|'eR|'ve|'VE|'vE|'Ve|'m|'M|'ll|'lL|'Ll|'LL|'d|'D)?"
const char* const kRegexO200k =
    "[^\r\n\\p{L}\\p{N}]?[\\p{Lu}\\p{Lt}\\p{Lm}\\p{Lo}\\p{M}]*[\\p{Ll}\\p{Lm}\\p{Lo}\\p{M}]+" TKZ_O2_SUFFIX
    "|[^\r\n\\p{L}\\p{N}]?[\\p{Lu}\\p{Lt}\\p{Lm}\\p{Lo}\\p{M}]+[\\p{Ll}\\p{Lm}\\p{Lo}\\p{M}]*" TKZ_O2_SUFFIX
    "|\\p{N}{1,3}| ?[^\\s\\p{L}\\p{N}]+[\\r\\n/]*|\\s*[\\r\\n]+|\\s+(?!\\S)|\\s+";

}  // namespace

extern "C" {

const char* tkz_last_error(void) { return g_err.c_str(); }

tkz_status tkz_vocab_from_tiktoken(const uint8_t* file, size_t n, tkz_vocab** out) {
    if (!out || (!file && n)) return fail(TKZ_E_ARG, "null argument");
    *out = nullptr;
    tkz_vocab* v = new tkz_vocab();
    std::string msg;
    int r = tkz::parse_tiktoken(file, n, &v->v, &msg);
    if (r == TKZ_OK) r = tkz::build_tables(&v->v, &msg);
    if (r != TKZ_OK) { delete v; return fail((tkz_status)r, msg); }
    *out = v;
    return TKZ_OK;
}
void tkz_vocab_destroy(tkz_vocab* v) { delete v; }
int64_t tkz_vocab_size(const tkz_vocab* v) { return v ? (int64_t)v->v.keys.size() : 0; }
int32_t tkz_vocab_max_key_len(const tkz_vocab* v) { return v ? v->v.max_key_len : 0; }
int64_t tkz_vocab_pair_table_entries(const tkz_vocab* v) { return v ? v->v.pair_entries : 0; }
int64_t tkz_vocab_table_bytes(const tkz_vocab* v, int32_t which) {
    if (!v) return 0;
    const tkz::Vocab& V = v->v;
    const int64_t b[5] = {(int64_t)(V.short_slots.size() * sizeof(TkzShortSlot)), (int64_t)(V.mid_slots.size() * sizeof(TkzMidSlot)),
                          (int64_t)(V.long_slots.size() * sizeof(TkzLongSlot) + V.long_blob.size()), (int64_t)(V.pair_slots.size() * sizeof(TkzPairSlot)),
                          (int64_t)((V.byte_rank.size() + V.bytepair_rank.size()) * sizeof(int32_t))};
    if (which == -1) return b[0] + b[1] + b[2] + b[3] + b[4];
    return which >= 0 && which < 5 ? b[which] : 0;
}
int32_t tkz_vocab_rank(const tkz_vocab* v, const uint8_t* key, int32_t len) {
    if (!v || len < 0 || (!key && len)) return -1;
    int32_t r;
    return v->v.lookup(std::string(reinterpret_cast<const char*>(key), (size_t)len), &r) ? r : -1;
}

void tkz_unicode_classes(uint32_t first, int32_t n, uint8_t* out) {
    const uint8_t* ucd = tkz::bmp_class_table().data();
    for (int32_t i = 0; out && i < n; ++i) out[i] = tkz_supp_class(ucd, first + (uint32_t)i);
}

tkz_status tkz_encoder_unicode_classes(tkz_encoder* e, uint32_t first, int32_t n, uint8_t* out) {
    // the table image as the DEVICE holds it (downloaded, then read as the kernels read it): a check of the upload, not of the host copy
    if (!out || n < 0) return fail(TKZ_E_ARG, "bad argument");
    DeviceScope scope;
    tkz_status st = check_encoder(e, scope);
    if (st != TKZ_OK) return st;
    std::vector<uint8_t> img(e->bmp_image_bytes);
    HIP_TRY(hipMemcpy(img.data(), e->t_bmp.p, img.size(), hipMemcpyDeviceToHost));
    for (int32_t i = 0; i < n; ++i) out[i] = tkz_supp_class(img.data(), first + (uint32_t)i);
    return TKZ_OK;
}

tkz_status tkz_encoder_set_unicode_classes(tkz_encoder* e, const uint8_t* classes, int64_t n_code_points) {
    // The split regexes are whatever the HOST's regex engine makes of \p{L}, \p{N}, \s: the reference compiles them with the running process's
    // System.Text.RegularExpressions (TikTokenizer.cs:77), whose Unicode data is the runtime's (13.0 under net6.0, 15.0 under .NET 8).  A host hands its
    // own classification over here; classes == NULL puts the built-in Unicode 13.0 table back.
    DeviceScope scope;
    tkz_status st = check_encoder(e, scope);
    if (st != TKZ_OK) return st;
    if (classes && n_code_points != 0x10000 && n_code_points != 0x110000) return fail(TKZ_E_ARG, "n_code_points must be 65536 (the BMP: code units) or 1114112 (every code point)");
    std::vector<uint8_t> img = tkz::bmp_class_table();                 // [TKZ_UCD_DIRECT direct classes][n][n x {first, last | class << 24}]
    if (classes) {
        for (int64_t cp = 0; cp < n_code_points; ++cp) if (classes[cp] > 8) return fail(TKZ_E_ARG, "a class code above 8 (0 other, 1 Lu, 2 Ll, 3 Lt, 4 Lm, 5 Lo, 6 M, 7 N, 8 white space)");
        // (the ASCII range keeps its classes: the scanners' fast paths know them; and a surrogate code unit is never a letter, digit or space)
        const int64_t direct = std::min<int64_t>(n_code_points, (int64_t)TKZ_UCD_DIRECT);
        for (int64_t cp = 128; cp < direct; ++cp) img[(size_t)cp] = (cp >= 0xD800 && cp <= 0xDFFF) ? 0 : classes[cp];
        if (n_code_points > (int64_t)TKZ_UCD_DIRECT) {
            std::vector<uint32_t> hi;
            for (int64_t cp = TKZ_UCD_DIRECT; cp < n_code_points;) {
                if (!classes[cp]) { ++cp; continue; }
                int64_t end = cp;
                while (end + 1 < n_code_points && classes[end + 1] == classes[cp]) ++end;
                hi.push_back((uint32_t)cp); hi.push_back((uint32_t)end | ((uint32_t)classes[cp] << 24));
                cp = end + 1;
            }
            if (hi.size() / 2 > 4096) return fail(TKZ_E_UNSUPPORTED, "more than 4096 classified ranges above U+3FFFF");
            const uint32_t n = (uint32_t)(hi.size() / 2);
            hi.insert(hi.begin(), n);
            img.resize(TKZ_UCD_DIRECT + hi.size() * 4);
            memcpy(img.data() + TKZ_UCD_DIRECT, hi.data(), hi.size() * 4);
        }
    }
    std::lock_guard<std::mutex> lock(e->mu);
    for (Workspace* w : e->pool) if (w->busy) return fail(TKZ_E_ARG, "the class table can only be replaced while no call of this encoder is in flight");
    if (hipDeviceSynchronize() != hipSuccess) return fail(TKZ_E_DEVICE, "hipDeviceSynchronize");
    const hipError_t h = upload(e->t_bmp, img, &e->bytes_allocated);
    if (h != hipSuccess) return fail(TKZ_E_DEVICE, std::string("class table upload: ") + hipGetErrorString(h));
    e->bmp_image_bytes = img.size();
    e->T.bmp_class = e->t_bmp.as<uint8_t>();
    return TKZ_OK;
}

tkz_status tkz_pattern_from_regex_engine(const char* regex_utf8, int32_t engine, int32_t* pattern_out) {
    if (!regex_utf8 || !pattern_out) return fail(TKZ_E_ARG, "null argument");
    if (engine != TKZ_ENGINE_DOTNET && engine != TKZ_ENGINE_ECMASCRIPT) return fail(TKZ_E_ARG, "unknown regex engine id");
    int32_t p = 0;
    if (!strcmp(regex_utf8, kRegexP1)) p = TKZ_PATTERN_P1;
    else if (!strcmp(regex_utf8, kRegexCl100k)) p = TKZ_PATTERN_CL100K;
    else if (!strcmp(regex_utf8, kRegexO200k)) p = engine == TKZ_ENGINE_ECMASCRIPT ? TKZ_PATTERN_O200K : TKZ_PATTERN_O200K_DOTNET;
    else return fail(TKZ_E_UNSUPPORTED, "only the three split patterns the reference defines are implemented (pattern 1, cl100k_base, o200k_base)");
    if (engine == TKZ_ENGINE_ECMASCRIPT && p != TKZ_PATTERN_O200K)
        return fail(TKZ_E_UNSUPPORTED, "pattern 1 and cl100k_base are implemented with the semantics of the C# reference's engine only (UTF-16 code units, .NET \\s)");
    *pattern_out = p;
    return TKZ_OK;
}
tkz_status tkz_pattern_from_regex(const char* regex_utf8, int32_t* pattern_out) {
    return tkz_pattern_from_regex_engine(regex_utf8, TKZ_ENGINE_DOTNET, pattern_out);
}

tkz_status tkz_encoder_create(const tkz_vocab* v, int32_t pattern, int32_t device, tkz_encoder** out) {
    if (!out || !v) return fail(TKZ_E_ARG, "null argument");
    *out = nullptr;
    if (pattern < TKZ_PATTERN_P1 || pattern > TKZ_PATTERN_O200K_DOTNET) return fail(TKZ_E_UNSUPPORTED, "unknown pattern id");
    int ndev = 0;
    hipError_t r = hipGetDeviceCount(&ndev);
    if (r != hipSuccess || ndev <= 0) return fail(TKZ_E_NO_DEVICE, "no HIP device available (libtkz has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(TKZ_E_ARG, "device index out of range");
    DeviceScope scope;
    HIP_TRY(scope.enter(device));
    tkz_encoder* e = new tkz_encoder();
    e->device = device; e->pattern = pattern; e->max_key_len = v->v.max_key_len;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess) e->small_ok = prop.sharedMemPerBlock >= (size_t)tkz::kSmallLdsBytesNeeded; }
    int64_t* acc = &e->bytes_allocated;
    const tkz::Vocab& V = v->v;
    hipError_t h = hipSuccess;
    // SHORT and MID in ONE allocation (k_probe addresses both from one uniform base with 32-bit offsets)
    const size_t short_bytes = V.short_slots.size() * sizeof(TkzShortSlot), mid_bytes = V.mid_slots.size() * sizeof(TkzMidSlot);
    if (h == hipSuccess) h = e->t_short.ensure(std::max<size_t>(64, short_bytes + mid_bytes), acc);
    if (h == hipSuccess && short_bytes) h = hipMemcpy(e->t_short.p, V.short_slots.data(), short_bytes, hipMemcpyHostToDevice);
    if (h == hipSuccess && mid_bytes) h = hipMemcpy(e->t_short.as<char>() + short_bytes, V.mid_slots.data(), mid_bytes, hipMemcpyHostToDevice);
    if (h == hipSuccess) h = upload(e->t_long, V.long_slots, acc);
    if (h == hipSuccess) h = upload(e->t_blob, V.long_blob, acc);
    if (h == hipSuccess) h = upload(e->t_pair, V.pair_slots, acc);
    if (h == hipSuccess) h = upload(e->t_byte, V.byte_rank, acc);
    if (h == hipSuccess) h = upload(e->t_bpair, V.bytepair_rank, acc);
    if (h == hipSuccess) h = upload(e->t_bmp, tkz::bmp_class_table(), acc);
    e->bmp_image_bytes = tkz::bmp_class_table().size();
    // {n_docs, n_bytes, n_tokens} of the last batch (tkz_encoder_counts_device): allocated once, here -- never from a call in flight
    if (h == hipSuccess) h = e->t_counts3.ensure(32, acc);
    if (h == hipSuccess) h = hipMemset(e->t_counts3.p, 0, 32);
    if (h != hipSuccess) { tkz_encoder_destroy(e); return fail(TKZ_E_DEVICE, std::string("table upload: ") + hipGetErrorString(h)); }
    e->T.short_slots = e->t_short.as<TkzShortSlot>(); e->T.short_nb = (uint32_t)(V.short_slots.size() / 2); e->T.short_seed = V.short_seed;
    e->T.mid_slots = reinterpret_cast<const TkzMidSlot*>(e->t_short.as<char>() + short_bytes); e->T.mid_ns = (uint32_t)V.mid_slots.size(); e->T.mid_seed = V.mid_seed;
    e->T.long_slots = e->t_long.as<TkzLongSlot>();    e->T.long_mask = (uint32_t)V.long_slots.size() - 1;
    e->T.long_blob = e->t_blob.as<uint8_t>();
    e->T.pair_slots = e->t_pair.as<TkzPairSlot>();    e->T.pair_n = (uint32_t)V.pair_slots.size(); e->T.pair_seed = V.pair_seed; e->T.pair_compact = V.pair_compact ? 1u : 0u;
    e->T.byte_rank = e->t_byte.as<int32_t>();
    e->T.bytepair_rank = e->t_bpair.as<int32_t>();
    e->T.bmp_class = e->t_bmp.as<uint8_t>();
    {   // the piece memo: 2^19 slots of 32 bytes (16 MB), empty
// (measured on the bench workload, k_merge_short per 5 GB: 2^15 slots 8.2 ms, 2^16 7.7, 2^17 7.1, 2^18 6.0, 2^19 5.4, 2^20 5.2, 2^22 8.4 -- the
//  hit rate grows with the table until it stops fitting the Infinity Cache beside everything else)
#ifndef TKZ_MEMO_SLOTS_LOG2
#define TKZ_MEMO_SLOTS_LOG2 19
#endif
        // ($TKZ_MEMO_SLOTS_LOG2 in the environment, 10..22: the tests' handle on it -- a memo that a few thousand pieces fill)
        uint32_t kMemoSlots = 1u << TKZ_MEMO_SLOTS_LOG2;
        { const char* v = getenv("TKZ_MEMO_SLOTS_LOG2"); const int n = v ? atoi(v) : 0; if (n >= 10 && n <= 22) kMemoSlots = 1u << n; }
        h = e->t_memo.ensure(size_t(kMemoSlots) * sizeof(TkzMemoSlot), acc);
        if (h == hipSuccess) h = hipMemset(e->t_memo.p, 0, size_t(kMemoSlots) * sizeof(TkzMemoSlot));
        if (h != hipSuccess) { tkz_encoder_destroy(e); return fail(TKZ_E_OUT_OF_MEMORY, std::string("piece memo: ") + hipGetErrorString(h)); }
        e->memo_slots = kMemoSlots;
        e->T.memo = e->t_memo.as<TkzMemoSlot>(); e->T.memo_n = kMemoSlots;
    }
    e->T.memo_hits = nullptr; e->T.memo_hits_sparse = 0; e->T.promo = nullptr; e->T.promo_n = 0;
    e->short_slots_n = (uint32_t)V.short_slots.size(); e->mid_slots_n = (uint32_t)V.mid_slots.size();
    e->T.max_key_len = V.max_key_len;
    e->T.pattern = pattern;
    e->T.max_rank = 0;
    for (int32_t r : V.ranks) e->T.max_rank = std::max(e->T.max_rank, r);
    e->dec_vocab.reserve(V.keys.size());
    for (size_t i = 0; i < V.keys.size(); ++i) e->dec_vocab.emplace_back(V.ranks[i], V.keys[i]);
    { const tkz_status ds = build_decode_table(e); if (ds != TKZ_OK) { tkz_encoder_destroy(e); return ds; } }
    *out = e;
    return TKZ_OK;
}

namespace {
void destroy_now(tkz_encoder* e);
}
void tkz_encoder_destroy(tkz_encoder* e) {
    if (!e) return;
    {   // handles of tkz_encode_batch_device_begin still outstanding: their _end calls need the encoder and its workspaces -- the last of
        // them frees it (and reports TKZ_E_ARG: the results of a batch whose encoder was destroyed under it are not to be trusted).
        // `destroyed` is set under the lock in either case, so that a _begin racing with this call is refused instead of leasing a
        // workspace of an encoder that is being deleted.
        std::lock_guard<std::mutex> lock(e->mu);
        if (e->destroyed) return;                       // (a second destroy while the first is deferred)
        e->destroyed = true;
        if (e->pending > 0) return;
    }
    destroy_now(e);
}
namespace {
void destroy_now(tkz_encoder* e) {
    join_promotion(e);
    DeviceScope scope;
    (void)scope.enter(e->device);
    DevBuf* bufs[] = {&e->t_short, &e->t_mid, &e->t_long, &e->t_blob, &e->t_pair, &e->t_byte, &e->t_bpair, &e->t_bmp, &e->t_counts3, &e->t_memo, &e->t_stats, &e->t_decoff, &e->t_decblob, &e->t_decids,
                      &e->t_memo_hits, &e->t_promo, &e->t_long_log, &e->t_lit};
    for (DevBuf* b : bufs) b->release();
    for (DevBuf& b : e->retired) b.release();
    for (Workspace* w : e->pool) { w->release_all(); delete w; }
    delete e;
}
}  // namespace
int32_t tkz_encoder_device(const tkz_encoder* e) { return e ? e->device : -1; }
const int64_t* tkz_encoder_counts_device(const tkz_encoder* e) { return e ? e->t_counts3.as<int64_t>() : nullptr; }

tkz_status tkz_host_alloc(size_t bytes, void** out) {
    if (!out) return fail(TKZ_E_ARG, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TKZ_E_NO_DEVICE, "no HIP device available");
    // (portable: page-locked for EVERY device of the process, whichever is current here -- a host with encoders on several GPUs hands the same
    //  buffers to any of them)
    const hipError_t r = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocPortable);
    if (r != hipSuccess) { *out = nullptr; return fail(TKZ_E_OUT_OF_MEMORY, std::string("hipHostMalloc: ") + hipGetErrorString(r)); }
    return TKZ_OK;
}
void tkz_host_free(void* p) { if (p) (void)hipHostFree(p); }

tkz_status tkz_encode_batch_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs,
                                 int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* needed) {
    return encode_host_batch(e, HostCall{bytes, nullptr, doc_offsets, n_docs, out_ids, out_cap, out_offsets, needed});
}

namespace {
// the `allowed` argument of the special entries -> the call's literal set, in the entry's *sc.  *sp: sc, or null -- nothing allowed or registered: the plain entry's call
tkz_status special_call(tkz_encoder* e, const int32_t* allowed, int32_t n_allowed, SpecialCall* sc, const SpecialCall** sp) {
    *sp = nullptr;
    if (!e) return fail(TKZ_E_ARG, "null encoder");
    if (n_allowed < 0 || (n_allowed > 0 && !allowed)) return fail(TKZ_E_ARG, "bad allowed-special arguments");
    std::lock_guard<std::mutex> lock(e->mu);
    if (n_allowed == 0 || e->lit_state == 0) return TKZ_OK;
    if (e->lit_state < 0) return fail(TKZ_E_UNSUPPORTED, "special tokens on the device: " + e->lit_why);
    *sc = SpecialCall{};
    sc->fffd = e->lit_fffd;
    for (int32_t k = 0; k < n_allowed; ++k) {
        const int32_t i = allowed[k];
        if (i < 0 || i >= e->LIT.n) return fail(TKZ_E_ARG, "allowed[] holds an index that is not a registered special token");
        if ((sc->allowed.m[i >> 6] >> (i & 63)) & 1ull) return fail(TKZ_E_ARG, "allowed[] holds an index twice");
        sc->allowed.m[i >> 6] |= 1ull << (i & 63);
    }
    *sp = sc;
    return TKZ_OK;
}
}  // namespace

tkz_status tkz_encode_batch_special_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                           const int32_t* allowed, int32_t n_allowed, int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets,
                                           void* hip_stream, int64_t* total_tokens) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    c.special = sp;
    return encode_device_batch(e, c, total_tokens);
}
tkz_status tkz_encode_batch_special_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed,
                                         int32_t n_allowed, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* needed) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    HostCall c{bytes, nullptr, doc_offsets, n_docs, out_ids, out_cap, out_offsets, needed};
    c.special = sp;
    return encode_host_batch(e, c);
}
void tkz_encoder_special_stats(const tkz_encoder* e, int64_t* batches, int64_t* literals) {
    if (batches) *batches = e ? e->spec_batches.load() : 0;
    if (literals) *literals = e ? e->spec_literals.load() : 0;
}

tkz_status tkz_encode_batch_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs,
                                   int64_t total_bytes, int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets,
                                   void* hip_stream, int64_t* total_tokens) {
    return encode_device_batch(e, BatchCall{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)}, total_tokens);
}

// The same in two halves: _begin enqueues the batch on the stream and returns, _end waits for it and reports as tkz_encode_batch_device
// does (a batch that needs a larger buffer than the first attempt had is run again inside _end).  The call keeps a workspace of the
// encoder from _begin to _end: several batches can be in flight, on one stream or on several.
struct tkz_pending { tkz_encoder* e; Lease* lease; BatchCall call; };
tkz_status tkz_encode_batch_device_begin_counts(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs,
                                                int64_t total_bytes, int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets,
                                                void* hip_stream, int64_t* d_counts3, tkz_pending** pending) {
    if (!pending) return fail(TKZ_E_ARG, "null pending");
    *pending = nullptr;
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    c.d_counts3 = d_counts3;
    DeviceScope scope;
    TKZ_TRY(check_device_call(e, scope, c));
    { std::lock_guard<std::mutex> lock(e->mu); if (e->destroyed) return fail(TKZ_E_ARG, "encoder destroyed"); ++e->pending; }
    tkz_pending* p = new tkz_pending{e, new Lease(e), c};
    const tkz_status st = encode_device(e, p->lease->ws, p->call, kCallBegin, nullptr);
    if (st != TKZ_OK) {
        (void)hipStreamSynchronize(c.stream);
        delete p->lease; delete p;
        const std::string msg = g_err;
        bool last;
        { std::lock_guard<std::mutex> lock(e->mu); last = --e->pending == 0 && e->destroyed; }
        if (last) destroy_now(e);                       // (destroy arrived while this _begin was running and no other handle is left)
        g_err = msg;
        return st;
    }
    *pending = p;
    return TKZ_OK;
}
tkz_status tkz_encode_batch_device_begin(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs,
                                         int64_t total_bytes, int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets,
                                         void* hip_stream, tkz_pending** pending) {
    return tkz_encode_batch_device_begin_counts(e, d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, hip_stream, nullptr, pending);
}
const int64_t* tkz_pending_counts_device(const tkz_pending* p) {
    if (!p) return nullptr;
    return p->call.d_counts3 ? p->call.d_counts3 : p->lease->ws->w_counts3.as<int64_t>();
}
tkz_status tkz_encode_batch_device_end(tkz_pending* p, int64_t* total_tokens) {
    if (!p) return fail(TKZ_E_ARG, "null pending");
    tkz_status st;
    tkz_encoder* e = p->e;
    {
        DeviceScope scope;
        st = check_encoder(e, scope);
        bool dead;
        { std::lock_guard<std::mutex> lock(e->mu); dead = e->destroyed; }
        if (st == TKZ_OK && !dead)
            st = encode_device(e, p->lease->ws, p->call, kCallEnd, total_tokens);
        else {
            (void)hipStreamSynchronize(p->call.stream);
            if (st == TKZ_OK) st = fail(TKZ_E_ARG, "the encoder was destroyed while this batch was in flight");
        }
    }
    delete p->lease;
    delete p;
    bool last;
    { std::lock_guard<std::mutex> lock(e->mu); last = --e->pending == 0 && e->destroyed; }
    if (last) destroy_now(e);
    return st;
}

tkz_status tkz_encode_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, int32_t* out_ids, int64_t out_cap, int64_t* n_out) {
    if (len < 0 || !n_out) return fail(TKZ_E_ARG, "bad argument");
    const int64_t offs[2] = {0, len};
    int64_t oo[2] = {0, 0}, needed = 0;
    tkz_status st = encode_host(e, HostCall{text, nullptr, offs, 1, out_ids, out_cap, oo, &needed});
    *n_out = needed;
    return st;
}

namespace {
// Encoding.UTF8.GetBytes semantics: a surrogate pair -> 4 bytes, a lone surrogate -> U+FFFD (EF BF BD).
// Splitting is unaffected: a lone surrogate (Cs) and U+FFFD (So) are both one "other" unit under every pattern.
// repl: null, or receives the replaced-byte bitmap over the bytes written (size / 64 + 1 words): one bit at the EF of every U+FFFD that stands for a lone
// surrogate -- what launch_u16_write leaves on the device, for the literal search of a special call (the reference searches the UTF-16 string).
void utf16_to_utf8(const uint16_t* text, int64_t len, std::vector<uint8_t>* out, std::vector<uint64_t>* repl) {
    std::vector<uint8_t>& u8 = *out;
    u8.clear();
    u8.reserve((size_t)len * 3);
    std::vector<size_t> lone;
    for (int64_t i = 0; i < len; ++i) {
        uint32_t c = text[i];
        if (c >= 0xD800 && c <= 0xDBFF && i + 1 < len && text[i + 1] >= 0xDC00 && text[i + 1] <= 0xDFFF) {
            c = 0x10000 + ((c - 0xD800) << 10) + (text[i + 1] - 0xDC00); ++i;
        } else if (c >= 0xD800 && c <= 0xDFFF) { c = 0xFFFD; if (repl) lone.push_back(u8.size()); }
        if (c < 0x80) u8.push_back((uint8_t)c);
        else if (c < 0x800) { u8.push_back(0xC0 | (c >> 6)); u8.push_back(0x80 | (c & 0x3F)); }
        else if (c < 0x10000) { u8.push_back(0xE0 | (c >> 12)); u8.push_back(0x80 | ((c >> 6) & 0x3F)); u8.push_back(0x80 | (c & 0x3F)); }
        else { u8.push_back(0xF0 | (c >> 18)); u8.push_back(0x80 | ((c >> 12) & 0x3F)); u8.push_back(0x80 | ((c >> 6) & 0x3F)); u8.push_back(0x80 | (c & 0x3F)); }
    }
    if (repl) {
        repl->assign(u8.size() / 64 + 1, 0ull);
        for (size_t p : lone) (*repl)[p >> 6] |= 1ull << (p & 63);
    }
}
}  // namespace

tkz_status tkz_encode_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, int32_t* out_ids, int64_t out_cap, int64_t* n_out) {
    if (len < 0 || (!text && len) || !n_out) return fail(TKZ_E_ARG, "bad argument");
    std::vector<uint8_t> u8;
    utf16_to_utf8(text, len, &u8, nullptr);
    return tkz_encode_utf8(e, u8.data(), (int64_t)u8.size(), out_ids, out_cap, n_out);
}

// ITokenizer.Encode(text, allowedSpecial) on ONE string (TikTokenizer.cs:178-207): the batch special entry's result for a batch of that one document -- from
// the single-launch kernel's special form where the plain single entries take the single-launch kernel (small_eligible), from the batch path otherwise and when
// the kernel hands the call back.  Nothing allowed or registered: the plain single entry's call.
tkz_status tkz_encode_special_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t* out_ids, int64_t out_cap,
                                   int64_t* n_out) {
    if (len < 0 || !n_out) return fail(TKZ_E_ARG, "bad argument");
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    if (!sp) return tkz_encode_utf8(e, text, len, out_ids, out_cap, n_out);
    const int64_t offs[2] = {0, len};
    int64_t oo[2] = {0, 0}, needed = 0;
    HostCall c{text, nullptr, offs, 1, out_ids, out_cap, oo, &needed};
    c.special = sp; c.single = true;
    const tkz_status st = encode_host(e, c);
    if (st == TKZ_OK) ++e->spec_batches;
    *n_out = needed;
    return st;
}

// The same for a UTF-16 string.  The host transcodes it as tkz_encode_utf16 does -- and, when a registered literal holds U+FFFD, notes where a U+FFFD stands for
// a lone surrogate -- for the single-launch kernel; a call that does not take it, or that the kernel hands back, is the batch entry's with the code units.
tkz_status tkz_encode_special_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t* out_ids, int64_t out_cap,
                                    int64_t* n_out) {
    if (len < 0 || (!text && len) || !n_out) return fail(TKZ_E_ARG, "bad argument");
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    if (!sp) return tkz_encode_utf16(e, text, len, out_ids, out_cap, n_out);
    std::vector<uint8_t> u8;
    std::vector<uint64_t> repl;
    utf16_to_utf8(text, len, &u8, sp->fffd ? &repl : nullptr);
    const int64_t offs[2] = {0, len}, offs8[2] = {0, (int64_t)u8.size()};
    int64_t oo[2] = {0, 0}, needed = 0;
    HostCall c8{u8.data(), nullptr, offs8, 1, out_ids, out_cap, oo, &needed};
    c8.special = sp; c8.single = true; c8.repl = sp->fffd ? repl.data() : nullptr;
    HostCall c{nullptr, text, offs, 1, out_ids, out_cap, oo, &needed};
    c.utf16 = true; c.special = sp; c.single = true; c.small_form = &c8;
    const tkz_status st = encode_host(e, c);
    if (st == TKZ_OK) ++e->spec_batches;
    *n_out = needed;
    return st;
}

tkz_status tkz_encode_batch_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs,
                                  int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* needed) {
    return encode_host_batch_utf16(e, units, unit_offsets, n_docs, nullptr, out_ids, out_cap, out_offsets, needed);
}

tkz_status tkz_encode_batch_special_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed,
                                          int32_t n_allowed, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* needed) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    return encode_host_batch_utf16(e, units, unit_offsets, n_docs, sp, out_ids, out_cap, out_offsets, needed);
}

// ---- count calls: the token offsets of an encode call and no ids (k_tokcount where k_place stands; the single-launch kernel as it is) ----
namespace {
// a count call that succeeded, and whether the single launch answered it
tkz_status count_done(tkz_encoder* e, tkz_status st, bool single) {
    if (st == TKZ_OK) { ++e->count_calls; if (single) ++e->count_single; }
    return st;
}
}  // namespace

tkz_status tkz_count_batch_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                  const int32_t* allowed, int32_t n_allowed, int64_t* d_out_offsets, void* hip_stream, int64_t* total_tokens) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, nullptr, 0, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    c.special = sp; c.count_only = true;
    return count_done(e, encode_device_batch(e, c, total_tokens), false);
}
tkz_status tkz_count_batch_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                int64_t* out_offsets, int64_t* total_tokens) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    bool single = false;
    HostCall c{bytes, nullptr, doc_offsets, n_docs, nullptr, 0, out_offsets, total_tokens};
    c.special = sp; c.count_only = true; c.took_single = &single;
    const tkz_status st = encode_host_batch(e, c);
    return count_done(e, st, single);
}
tkz_status tkz_count_batch_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                 int64_t* out_offsets, int64_t* total_tokens) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    return count_done(e, encode_host_batch_utf16(e, units, unit_offsets, n_docs, sp, nullptr, 0, out_offsets, total_tokens, true), false);
}
// ONE text: the routes of tkz_encode_utf8 / tkz_encode_special_utf8 (the single-launch kernel where they take it, its special form for a text with literals)
tkz_status tkz_count_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t* n_out) {
    if (len < 0 || !n_out) return fail(TKZ_E_ARG, "bad argument");
    *n_out = 0;
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    const int64_t offs[2] = {0, len};
    int64_t oo[2] = {0, 0}, needed = 0;
    bool single = false;
    HostCall c{text, nullptr, offs, 1, nullptr, 0, oo, &needed};
    c.special = sp; c.single = sp != nullptr; c.count_only = true; c.took_single = &single;
    const tkz_status st = encode_host(e, c);
    if (st == TKZ_OK && sp) ++e->spec_batches;
    if (st == TKZ_OK) *n_out = oo[1];
    return count_done(e, st, single);
}
// ... a UTF-16 string: transcoded on the host, as tkz_encode_utf16 / tkz_encode_special_utf16 do
tkz_status tkz_count_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t* n_out) {
    if (len < 0 || (!text && len) || !n_out) return fail(TKZ_E_ARG, "bad argument");
    *n_out = 0;
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    std::vector<uint8_t> u8;
    std::vector<uint64_t> repl;
    utf16_to_utf8(text, len, &u8, sp && sp->fffd ? &repl : nullptr);
    if (!sp) return tkz_count_utf8(e, u8.data(), (int64_t)u8.size(), nullptr, 0, n_out);
    const int64_t offs[2] = {0, len}, offs8[2] = {0, (int64_t)u8.size()};
    int64_t oo[2] = {0, 0}, needed = 0;
    bool single = false;
    HostCall c8{u8.data(), nullptr, offs8, 1, nullptr, 0, oo, &needed};
    c8.special = sp; c8.single = true; c8.repl = sp->fffd ? repl.data() : nullptr; c8.count_only = true; c8.took_single = &single;
    HostCall c{nullptr, text, offs, 1, nullptr, 0, oo, &needed};
    c.utf16 = true; c.special = sp; c.single = true; c.small_form = &c8; c.count_only = true;
    const tkz_status st = encode_host(e, c);
    if (st == TKZ_OK) { ++e->spec_batches; *n_out = oo[1]; }
    return count_done(e, st, single);
}
void tkz_encoder_count_calls(const tkz_encoder* e, int64_t* calls, int64_t* single_launch) {
    if (calls) *calls = e ? e->count_calls.load() : 0;
    if (single_launch) *single_launch = e ? e->count_single.load() : 0;
}


tkz_status tkz_pretokenize_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, uint64_t* out_bitmap_words) {
    if (!out_bitmap_words) return fail(TKZ_E_ARG, "null output buffer");
    HostCall c{bytes, nullptr, doc_offsets, n_docs, nullptr, 0, nullptr, nullptr};
    c.kind = CallKind::BitmapOnly; c.bitmap = out_bitmap_words;
    return encode_host(e, c);
}

tkz_status tkz_encode_pieces(tkz_encoder* e, const uint8_t* bytes, const int64_t* piece_offsets, int64_t n_pieces,
                             int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* needed) {
    HostCall c{bytes, nullptr, piece_offsets, n_pieces, out_ids, out_cap, out_offsets, needed};
    c.kind = CallKind::OnePiecePerDoc;
    return encode_host_batch(e, c);
}

tkz_status tkz_encode_batch_pieces_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs,
                                        int32_t* out_ids, int64_t out_cap, int64_t* doc_piece_offsets, int64_t* piece_byte_offsets,
                                        int64_t* piece_token_offsets, int64_t piece_cap, int64_t* n_pieces, int64_t* needed_ids) {
    TKZ_TRY(check_host_outputs(out_ids, out_cap, doc_piece_offsets));
    if (!piece_byte_offsets || !piece_token_offsets || !n_pieces) return fail(TKZ_E_ARG, "null output buffer");
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(doc_offsets, n_docs, bytes != nullptr, kSizedDocs, &total));
    if (piece_cap < 0) return fail(TKZ_E_ARG, kSizedDocs.negative);
    *n_pieces = 0;
    if (needed_ids) *needed_ids = 0;
    if (total == 0) {                                        // no bytes: no pieces (empty documents have none)
        TKZ_TRY(check_empty_docs(doc_offsets, n_docs, kSizedDocs, doc_piece_offsets));
        piece_byte_offsets[0] = 0; piece_token_offsets[0] = 0;
        return TKZ_OK;
    }
    // ONE launch sequence on the device: Regex.Matches -> piece offsets from the bitmap -> encode with a token mark per piece
    Lease lease(e);
    Workspace* ws = lease.ws;
    const int64_t pcap = std::min<int64_t>(piece_cap, total);           // pieces <= bytes
    const int64_t cap = std::min<int64_t>(out_cap, total);
    TKZ_TRY(stage_in(ws, bytes, total, doc_offsets, n_docs));
    TKZ_TRY(stage_out(ws, n_docs, cap, false));
    for (DevBuf* b : {&ws->p_boffs, &ws->p_toffs}) HIP_TRY(b->ensure((size_t)(pcap + 1) * 8, &ws->bytes_allocated));
    HIP_TRY(ws->p_docp.ensure((size_t)(n_docs + 1) * 8, &ws->bytes_allocated));
    PiecesOut po{ws->p_boffs.as<int64_t>(), ws->p_toffs.as<int64_t>(), ws->p_docp.as<int64_t>(), pcap, 0};
    int64_t tokens = 0;
    BatchCall c = staged_call(ws, n_docs, total, cap);
    c.d_out_offs = nullptr; c.kind = CallKind::Pieces; c.pieces = &po;
    const tkz_status st = encode_device(e, ws, c, kCallWhole, &tokens);
    *n_pieces = po.n_pieces;
    if (needed_ids) *needed_ids = tokens;
    if (st != TKZ_OK) return st;
    TKZ_TRY(fetch(ws, out_ids, tokens, nullptr, n_docs));
    HIP_TRY(hipMemcpy(piece_byte_offsets, ws->p_boffs.p, (size_t)(po.n_pieces + 1) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(piece_token_offsets, ws->p_toffs.p, (size_t)(po.n_pieces + 1) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(doc_piece_offsets, ws->p_docp.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost));
    return TKZ_OK;
}

// ---- EncodeTrimSuffix / EncodeTrimPrefix for a batch (TikTokenizer.cs:288-579) ------------------------

namespace {
// the trim call on device buffers, on a workspace the entry holds: the piece-granular launch sequence with the piece arrays and the untrimmed ids in the
// workspace, then the cut, the scan and the kept ids (enqueue_attempt)
tkz_status trim_on_device(tkz_encoder* e, Workspace* ws, BatchCall c, const TrimCall& tc, const SpecialCall* sc, int64_t* total_tokens) {
    int64_t* acc = &ws->bytes_allocated;
    PiecesOut po{nullptr, nullptr, nullptr, c.total, 0};                // (pieces <= bytes: the arrays are sized once the pieces are counted)
    if (c.total > 0) {
        HIP_TRY(ws->p_docp.ensure((size_t)(c.n_docs + 1) * 8, acc));
        HIP_TRY(ws->t_ids.ensure((size_t)c.total * 4, acc));
        HIP_TRY(ws->t_keep.ensure((size_t)std::max<int64_t>(c.n_docs, 1) * 3 * 8, acc));
        HIP_TRY(ws->t_bsum.ensure((size_t)(c.n_docs / tkz::kScanBlock + 2) * 8, acc));
        po.doc_piece = ws->p_docp.as<int64_t>();
    }
    c.kind = CallKind::Trim; c.pieces = &po; c.trim = &tc; c.special = sc;
    const tkz_status st = encode_device(e, ws, c, kCallWhole, total_tokens);
    if (st == TKZ_OK && sc) ++e->spec_batches;
    return st;
}
tkz_status check_trim_args(int32_t side, int64_t max_tokens, bool per_doc, const int64_t* h_max = nullptr, int64_t n_docs = 0) {      // (h_max: the maxima, when in host memory)
    if (side != TKZ_TRIM_SUFFIX && side != TKZ_TRIM_PREFIX) return fail(TKZ_E_ARG, "side must be TKZ_TRIM_SUFFIX or TKZ_TRIM_PREFIX");
    if (!per_doc && max_tokens < 0) return fail(TKZ_E_ARG, "negative maximum token count");
    for (int64_t d = 0; h_max && d < n_docs; ++d) if (h_max[d] < 0) return fail(TKZ_E_ARG, "negative maximum token count");
    return TKZ_OK;
}
// The second half of a trim host entry, with the batch on the device as UTF-8 (c: its bytes and byte offsets): staging for the kept ids, their offsets and the
// per-document arrays (the maxima, the two cut arrays), ONE trim call, the results back.
tkz_status trim_staged(tkz_encoder* e, Workspace* ws, BatchCall c, int32_t side, int64_t max_tokens, const int64_t* per_doc, const SpecialCall* sp,
                       int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* cut_bytes, int64_t* cut_units, int64_t* needed) {
    const int64_t n_docs = c.n_docs, nd = std::max<int64_t>(n_docs, 1);
    c.out_cap = std::min<int64_t>(out_cap, c.total);
    TKZ_TRY(stage_out(ws, n_docs, c.out_cap));
    HIP_TRY(ws->t_stage.ensure((size_t)nd * 3 * 8, &ws->bytes_allocated));
    int64_t* const d_max = ws->t_stage.as<int64_t>(), * const d_cb = d_max + nd, * const d_cu = d_cb + nd;
    if (per_doc && n_docs) HIP_TRY(hipMemcpy(d_max, per_doc, (size_t)n_docs * 8, hipMemcpyHostToDevice));
    c.d_out = ws->s_out[0].as<int32_t>(); c.d_out_offs = ws->s_outoffs[0].as<int64_t>();
    int64_t tokens = 0;
    const tkz_status st = trim_on_device(e, ws, c, TrimCall{side, max_tokens, per_doc ? d_max : nullptr, cut_bytes ? d_cb : nullptr, cut_units ? d_cu : nullptr}, sp, &tokens);
    if (needed) *needed = tokens;
    if (st != TKZ_OK) return st;
    TKZ_TRY(fetch(ws, out_ids, tokens, out_offsets, n_docs));
    if (cut_bytes && n_docs) HIP_TRY(hipMemcpy(cut_bytes, d_cb, (size_t)n_docs * 8, hipMemcpyDeviceToHost));
    if (cut_units && n_docs) HIP_TRY(hipMemcpy(cut_units, d_cu, (size_t)n_docs * 8, hipMemcpyDeviceToHost));
    return TKZ_OK;
}
}  // namespace

tkz_status tkz_encode_batch_trim_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                        const int32_t* allowed, int32_t n_allowed, int32_t side, int64_t max_tokens, const int64_t* d_max_tokens,
                                        int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets, int64_t* d_cut_bytes, int64_t* d_cut_units,
                                        void* hip_stream, int64_t* total_tokens) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_trim_args(side, max_tokens, d_max_tokens != nullptr));
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    // (a call that can keep nothing -- a maximum of 0 -- needs no id buffer)
    if (!d_doc_offsets || !d_out_offsets || (total_bytes > 0 && !d_bytes) || (out_cap > 0 && !d_out_ids)) return fail(TKZ_E_ARG, "null device buffer");
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(TKZ_E_ARG, "d_bytes must be 16-byte aligned");
    Lease lease(e);
    return trim_on_device(e, lease.ws, c, TrimCall{side, max_tokens, d_max_tokens, d_cut_bytes, d_cut_units}, sp, total_tokens);
}

tkz_status tkz_encode_batch_trim_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                      int32_t side, int64_t max_tokens, const int64_t* max_tokens_per_doc, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                      int64_t* cut_bytes, int64_t* cut_units, int64_t* needed) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_trim_args(side, max_tokens, max_tokens_per_doc != nullptr, max_tokens_per_doc, n_docs));
    TKZ_TRY(check_host_outputs(out_ids, out_cap, out_offsets, "null output buffer", false));
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(doc_offsets, n_docs, bytes != nullptr, kSizedDocs, &total));
    if (total == 0) TKZ_TRY(check_empty_docs(doc_offsets, n_docs, kSizedDocs, nullptr));      // (... and the device call runs all the same)
    if (needed) *needed = 0;
    // the whole batch is staged (as tkz_encode_batch_pieces_utf8 stages it) and the result copied from ONE call of the device entry
    Lease lease(e);
    Workspace* ws = lease.ws;
    TKZ_TRY(stage_in(ws, bytes, total, doc_offsets, n_docs));
    return trim_staged(e, ws, staged_call(ws, n_docs, total, 0), side, max_tokens, max_tokens_per_doc, sp, out_ids, out_cap, out_offsets, cut_bytes, cut_units, needed);
}

// The same for UTF-16 documents: the whole batch's code units are staged and transcoded on the device (as a chunk of tkz_encode_batch_utf16 is), then ONE trim call
// on the UTF-8 bytes and byte offsets that leaves.  With a registered literal that holds U+FFFD the transcoder also writes the replaced-byte bitmap.
tkz_status tkz_encode_batch_trim_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                       int32_t side, int64_t max_tokens, const int64_t* max_tokens_per_doc, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                       int64_t* cut_units, int64_t* needed) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_trim_args(side, max_tokens, max_tokens_per_doc != nullptr, max_tokens_per_doc, n_docs));
    TKZ_TRY(check_host_outputs(out_ids, out_cap, out_offsets, "null output buffer", false));
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(unit_offsets, n_docs, units != nullptr, kUnitDocs, &total));
    if (needed) *needed = 0;
    if (total == 0) {
        TKZ_TRY(check_empty_docs(unit_offsets, n_docs, kUnitDocs, out_offsets));
        if (cut_units) std::fill_n(cut_units, n_docs, int64_t(0));
        if (sp) ++e->spec_batches;                                      // (the one counted special batch that does not reach trim_on_device)
        return TKZ_OK;
    }
    // (the workspace keeps what is taken here for its next call; the lease -- and with it every buffer's use -- ends with this frame on every return)
    Lease lease(e);
    Workspace* ws = lease.ws;
    U16Stage& U = ws->u16[0];
    const bool with_repl = sp && sp->fffd;
    HIP_TRY(U.ensure(total, n_docs, &ws->bytes_allocated, with_repl));
    HIP_TRY(hipMemcpy(U.units.p, units, (size_t)total * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U.offs.p, unit_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    const tkz::Launch L{nullptr, nullptr, ws};
    HIP_TRY(u16_measure(U, L, total, n_docs));
    HIP_TRY(hipStreamSynchronize(nullptr));
    int64_t nbytes = 0;                                                 // the batch as UTF-8
    TKZ_TRY(u16_write(U, L, total, n_docs, with_repl, &ws->bytes_allocated, &nbytes));
    BatchCall c{U.bytes.as<uint8_t>(), U.boffs.as<int64_t>(), n_docs, nbytes, nullptr, 0, nullptr, nullptr};
    if (with_repl) c.d_repl = U.repl.as<uint64_t>();
    return trim_staged(e, ws, c, side, max_tokens, max_tokens_per_doc, sp, out_ids, out_cap, out_offsets, nullptr, cut_units, needed);
}

// ---- EncodeTrimSuffix / EncodeTrimPrefix on ONE string: the batch trim entries' result for a batch of that one document and a uniform maximum -- from the
// single-launch kernel's trim form where the plain single entries take the single-launch kernel (small_eligible) and the text has at most kSmallTrimMaxBytes
// bytes, from the batch trim entries otherwise and when the kernel hands the call back ----

namespace {
// the launch for the text as UTF-8 (c8: single, with its TrimOne).  *handled false: the text is not eligible, or the kernel handed it back
tkz_status trim_small(tkz_encoder* e, const HostCall& c8, bool* handled) {
    *handled = false;
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    if (c8.total() > tkz::kSmallTrimMaxBytes || !small_eligible(e, c8.offs, 1, c8.total())) return TKZ_OK;     // (beyond it the batch trim path is as fast or faster; UTF-16: the bytes may exceed it)
    Lease lease(e);
    const tkz_status st = encode_small(e, lease.ws, c8, handled);
    if (st == TKZ_OK && *handled && c8.special) ++e->spec_batches;
    return st;
}
}  // namespace

tkz_status tkz_encode_trim_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t side, int64_t max_tokens,
                                int32_t* out_ids, int64_t out_cap, int64_t* n_out, int64_t* cut_bytes, int64_t* cut_units) {
    if (len < 0 || (!text && len) || !n_out) return fail(TKZ_E_ARG, "bad argument");
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_trim_args(side, max_tokens, false));
    const int64_t offs[2] = {0, len};
    int64_t oo[2] = {0, 0}, needed = 0, cb = 0, cu = 0;
    TKZ_TRY(check_host_outputs(out_ids, out_cap, oo, "null output buffer", false));
    *n_out = 0;
    if (cut_bytes) *cut_bytes = 0;
    if (cut_units) *cut_units = 0;
    if (len == 0) { if (sp) ++e->spec_batches; return TKZ_OK; }
    const TrimOne t{side, max_tokens, &cb, &cu};
    HostCall c{text, nullptr, offs, 1, out_ids, out_cap, oo, &needed};
    c.special = sp; c.single = true; c.trim = &t;
    bool handled = false;
    tkz_status st = len <= tkz::kSmallTrimMaxBytes ? trim_small(e, c, &handled) : TKZ_OK;      // (a longer text costs nothing here before the batch entry has it)
    if (st == TKZ_OK && !handled)
        st = tkz_encode_batch_trim_utf8(e, text, offs, 1, allowed, n_allowed, side, max_tokens, nullptr, out_ids, out_cap, oo, &cb, &cu, &needed);
    *n_out = needed;
    if (cut_bytes) *cut_bytes = cb;
    if (cut_units) *cut_units = cu;
    return st;
}

// The same for a UTF-16 string.  The host transcodes it as tkz_encode_special_utf16 does -- the replaced-byte bitmap in the same loop when a registered literal
// holds U+FFFD -- for the single-launch kernel, whose unit count needs nothing more: a replacement is the one unit it stands for.  A call that does not take the
// launch, or that the kernel hands back, is the batch entry's with the code units.
tkz_status tkz_encode_trim_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t side, int64_t max_tokens,
                                 int32_t* out_ids, int64_t out_cap, int64_t* n_out, int64_t* cut_units) {
    if (len < 0 || (!text && len) || !n_out) return fail(TKZ_E_ARG, "bad argument");
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_trim_args(side, max_tokens, false));
    const int64_t offs[2] = {0, len};
    int64_t oo[2] = {0, 0}, needed = 0, cu = 0;
    TKZ_TRY(check_host_outputs(out_ids, out_cap, oo, "null output buffer", false));
    *n_out = 0;
    if (cut_units) *cut_units = 0;
    if (len == 0) { if (sp) ++e->spec_batches; return TKZ_OK; }
    tkz_status st = TKZ_OK;
    bool handled = false;
    // (a unit is a byte at least: a string that is not eligible at `len` BYTES -- too long, o200k beyond its 1 KiB, a device without the LDS -- is not eligible
    //  as the bytes it becomes, and is not transcoded here only to be transcoded again by the batch entry)
    if (len <= tkz::kSmallTrimMaxBytes && small_eligible(e, offs, 1, len)) {
        std::vector<uint8_t> u8;
        std::vector<uint64_t> repl;
        utf16_to_utf8(text, len, &u8, sp && sp->fffd ? &repl : nullptr);
        const int64_t offs8[2] = {0, (int64_t)u8.size()};
        const TrimOne t{side, max_tokens, nullptr, &cu};
        HostCall c8{u8.data(), nullptr, offs8, 1, out_ids, out_cap, oo, &needed};
        c8.special = sp; c8.single = true; c8.trim = &t; c8.repl = sp && sp->fffd ? repl.data() : nullptr;
        st = trim_small(e, c8, &handled);
    }
    if (st == TKZ_OK && !handled)
        st = tkz_encode_batch_trim_utf16(e, text, offs, 1, allowed, n_allowed, side, max_tokens, nullptr, out_ids, out_cap, oo, &cu, &needed);
    *n_out = needed;
    if (cut_units) *cut_units = cu;
    return st;
}

// ---- token spans: the ids and offsets of the matching encode entry, and where every token's text starts in its document (bytes, UTF-16 code units) ----

namespace {
// the span call on device buffers, on a workspace the entry holds: the piece-granular launch sequence with the piece arrays in the workspace and the ids in the
// caller's buffer, then the token starts (enqueue_attempt)
tkz_status spans_on_device(tkz_encoder* e, Workspace* ws, BatchCall c, const SpanCall& sc, const SpecialCall* sp, int64_t* total_tokens) {
    int64_t* acc = &ws->bytes_allocated;
    PiecesOut po{nullptr, nullptr, nullptr, c.total, 0};                // (pieces <= bytes: the arrays are sized once the pieces are counted)
    if (c.total > 0) {
        const int64_t nwords = c.total / 64 + 1, ntiles = (c.total + tkz::kSub - 1) / tkz::kSub;
        HIP_TRY(ws->p_docp.ensure((size_t)(c.n_docs + 1) * 8, acc));
        HIP_TRY(ws->sp_intbits.ensure((size_t)(nwords + 8) * 8, acc));
        HIP_TRY(ws->sp_cnt.ensure((size_t)ntiles * 2 * 4, acc));
        HIP_TRY(ws->sp_base.ensure((size_t)(ntiles * 2 + 2) * 8, acc));
        po.doc_piece = ws->p_docp.as<int64_t>();
    }
    c.kind = CallKind::Spans; c.pieces = &po; c.spans = &sc; c.special = sp;
    const tkz_status st = encode_device(e, ws, c, kCallWhole, total_tokens);
    if (st == TKZ_OK) { ++e->spans_calls; if (sp) ++e->spec_batches; }
    return st;
}
// The second half of a span host entry, with the batch on the device as UTF-8 (c: its bytes and byte offsets): staging for the ids, their offsets and the two span
// arrays, ONE span call, the results back.  A document of 2^31 bytes or more is refused from the byte offsets when the caller's were in bytes (h_offs), by the
// device otherwise.
tkz_status spans_staged(tkz_encoder* e, Workspace* ws, BatchCall c, const SpecialCall* sp, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                        int32_t* tok_bytes, int32_t* tok_units, int64_t* needed) {
    const int64_t n_docs = c.n_docs;
    c.out_cap = std::min<int64_t>(out_cap, c.total);
    const int64_t cap = std::max<int64_t>(c.out_cap, 1);
    TKZ_TRY(stage_out(ws, n_docs, c.out_cap));
    HIP_TRY(ws->sp_stage.ensure((size_t)cap * 2 * 4, &ws->bytes_allocated));
    int32_t* const d_tb = ws->sp_stage.as<int32_t>(), * const d_tu = d_tb + cap;
    c.d_out = ws->s_out[0].as<int32_t>(); c.d_out_offs = ws->s_outoffs[0].as<int64_t>();
    int64_t tokens = 0;
    const tkz_status st = spans_on_device(e, ws, c, SpanCall{tok_bytes ? d_tb : nullptr, tok_units ? d_tu : nullptr}, sp, &tokens);
    if (needed) *needed = tokens;
    if (st != TKZ_OK) return st;
    TKZ_TRY(fetch(ws, out_ids, tokens, out_offsets, n_docs));
    if (tok_bytes && tokens) HIP_TRY(hipMemcpy(tok_bytes, d_tb, (size_t)tokens * 4, hipMemcpyDeviceToHost));
    if (tok_units && tokens) HIP_TRY(hipMemcpy(tok_units, d_tu, (size_t)tokens * 4, hipMemcpyDeviceToHost));
    return TKZ_OK;
}
const char* const kMsgSpanArrays = "token spans: tok_bytes and tok_units are both null";
const char* const kMsgSpanDoc = "token spans: a document of 2^31 bytes or more";
}  // namespace

tkz_status tkz_encode_batch_spans_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                         const int32_t* allowed, int32_t n_allowed, int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets,
                                         int32_t* d_tok_bytes, int32_t* d_tok_units, void* hip_stream, int64_t* total_tokens) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    if (!d_tok_bytes && !d_tok_units) return fail(TKZ_E_ARG, kMsgSpanArrays);
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    DeviceScope scope;
    TKZ_TRY(check_device_call(e, scope, c));
    Lease lease(e);
    return spans_on_device(e, lease.ws, c, SpanCall{d_tok_bytes, d_tok_units}, sp, total_tokens);
}

tkz_status tkz_encode_batch_spans_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                       int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int32_t* tok_bytes, int32_t* tok_units, int64_t* needed) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    if (!tok_bytes && !tok_units) return fail(TKZ_E_ARG, kMsgSpanArrays);
    TKZ_TRY(check_host_outputs(out_ids, out_cap, out_offsets, "null output buffer", false));
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(doc_offsets, n_docs, bytes != nullptr, kSizedDocs, &total));
    if (total == 0) TKZ_TRY(check_empty_docs(doc_offsets, n_docs, kSizedDocs, nullptr));      // (... and the device call runs all the same)
    if (needed) *needed = 0;
    for (int64_t d = 0; d < n_docs; ++d) if (doc_offsets[d + 1] - doc_offsets[d] > (int64_t)INT32_MAX) return fail(TKZ_E_UNSUPPORTED, kMsgSpanDoc);
    // the whole batch is staged and the result copied from ONE call of the device entry, as tkz_encode_batch_trim_utf8 does
    Lease lease(e);
    Workspace* ws = lease.ws;
    TKZ_TRY(stage_in(ws, bytes, total, doc_offsets, n_docs));
    return spans_staged(e, ws, staged_call(ws, n_docs, total, 0), sp, out_ids, out_cap, out_offsets, tok_bytes, tok_units, needed);
}

// The same for UTF-16 documents: code units staged and transcoded on the device as tkz_encode_batch_trim_utf16 does; positions in code units only -- the bytes
// never exist on the host.
tkz_status tkz_encode_batch_spans_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                        int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int32_t* tok_units, int64_t* needed) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    if (!tok_units) return fail(TKZ_E_ARG, kMsgSpanArrays);
    TKZ_TRY(check_host_outputs(out_ids, out_cap, out_offsets, "null output buffer", false));
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(unit_offsets, n_docs, units != nullptr, kUnitDocs, &total));
    if (needed) *needed = 0;
    if (total == 0) {
        TKZ_TRY(check_empty_docs(unit_offsets, n_docs, kUnitDocs, out_offsets));
        ++e->spans_calls;
        if (sp) ++e->spec_batches;
        return TKZ_OK;
    }
    // (a unit is at most three bytes: a document of fewer than 2^31 / 3 units cannot reach 2^31 bytes; a longer one is measured by the device)
    Lease lease(e);
    Workspace* ws = lease.ws;
    U16Stage& U = ws->u16[0];
    const bool with_repl = sp && sp->fffd;
    HIP_TRY(U.ensure(total, n_docs, &ws->bytes_allocated, with_repl));
    HIP_TRY(hipMemcpy(U.units.p, units, (size_t)total * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U.offs.p, unit_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    const tkz::Launch L{nullptr, nullptr, ws};
    HIP_TRY(u16_measure(U, L, total, n_docs));
    HIP_TRY(hipStreamSynchronize(nullptr));
    int64_t nbytes = 0;                                                 // the batch as UTF-8
    TKZ_TRY(u16_write(U, L, total, n_docs, with_repl, &ws->bytes_allocated, &nbytes));
    BatchCall c{U.bytes.as<uint8_t>(), U.boffs.as<int64_t>(), n_docs, nbytes, nullptr, 0, nullptr, nullptr};
    if (with_repl) c.d_repl = U.repl.as<uint64_t>();
    return spans_staged(e, ws, c, sp, out_ids, out_cap, out_offsets, nullptr, tok_units, needed);
}

// ONE text: the batch entry with one document, at every size
tkz_status tkz_encode_spans_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t* out_ids, int64_t out_cap,
                                 int32_t* tok_bytes, int32_t* tok_units, int64_t* n_out) {
    if (len < 0 || !n_out) return fail(TKZ_E_ARG, "bad argument");
    *n_out = 0;
    const int64_t offs[2] = {0, len};
    int64_t oo[2] = {0, 0}, needed = 0;
    const tkz_status st = tkz_encode_batch_spans_utf8(e, text, offs, 1, allowed, n_allowed, out_ids, out_cap, oo, tok_bytes, tok_units, &needed);
    *n_out = needed;
    return st;
}
tkz_status tkz_encode_spans_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int32_t* out_ids, int64_t out_cap,
                                  int32_t* tok_units, int64_t* n_out) {
    if (len < 0 || (!text && len) || !n_out) return fail(TKZ_E_ARG, "bad argument");
    *n_out = 0;
    const int64_t offs[2] = {0, len};
    int64_t oo[2] = {0, 0}, needed = 0;
    const tkz_status st = tkz_encode_batch_spans_utf16(e, text, offs, 1, allowed, n_allowed, out_ids, out_cap, oo, tok_units, &needed);
    *n_out = needed;
    return st;
}
void tkz_encoder_spans_calls(const tkz_encoder* e, int64_t* calls) {
    if (calls) *calls = e ? e->spans_calls.load() : 0;
}

// ---- token-budget chunks: the ids and offsets of the matching encode entry, and every document's tokens cut into chunks of at most max_tokens (tkz.h: the rule) ----

namespace {
// the chunk call on device buffers, on a workspace the entry holds: the piece-granular launch sequence with the piece arrays in the workspace and the ids in the
// caller's buffer, then the two walks and the table (enqueue_attempt)
tkz_status chunks_on_device(tkz_encoder* e, Workspace* ws, BatchCall c, ChunkCall cc, const SpecialCall* sp, int64_t* total_tokens, int64_t* n_chunks) {
    int64_t* acc = &ws->bytes_allocated;
    int64_t chunks = 0;
    PiecesOut po{nullptr, nullptr, nullptr, c.total, 0};                // (pieces <= bytes: the arrays are sized once the pieces are counted)
    if (c.total > 0) {
        const int64_t nspan = (c.total + tkz::kChunkUnitSpan - 1) / tkz::kChunkUnitSpan;
        HIP_TRY(ws->p_docp.ensure((size_t)(c.n_docs + 1) * 8, acc));
        HIP_TRY(ws->ck_cnt.ensure((size_t)(c.n_docs + 1) * 8, acc));
        HIP_TRY(ws->ck_bsum.ensure((size_t)(c.n_docs / tkz::kScanBlock + 2) * 8, acc));
        HIP_TRY(ws->ck_list.ensure((size_t)std::max<int64_t>(c.n_docs, 1) * 8, acc));
        if (cc.wants_units()) {
            HIP_TRY(ws->ck_ucnt.ensure((size_t)nspan * 4, acc));
            HIP_TRY(ws->ck_ubase.ensure((size_t)(nspan + 2 + nspan / tkz::kScanBlock + 2) * 8, acc));      // (the bases, the total, the scan's partial sums)
        }
        po.doc_piece = ws->p_docp.as<int64_t>();
    }
    if (cc.max_tokens > (int64_t(1) << 62)) cc.max_tokens = int64_t(1) << 62;      // (s + max_tokens is computed on the device)
    cc.n_chunks = &chunks;
    c.kind = CallKind::Chunks; c.pieces = &po; c.chunks = &cc; c.special = sp;
    const tkz_status st = encode_device(e, ws, c, kCallWhole, total_tokens);
    if (n_chunks) *n_chunks = chunks;
    if (st == TKZ_OK) { ++(cc.overlap >= 0 ? e->chunks_overlap_calls : e->chunks_calls); if (sp) ++e->spec_batches; }
    return st;
}
// The second half of a chunk host entry, with the batch on the device as UTF-8 (c: its bytes and byte offsets): staging for the ids, their offsets and the table,
// ONE chunk call, the results back.
tkz_status chunks_staged(tkz_encoder* e, Workspace* ws, BatchCall c, int64_t max_tokens, const SpecialCall* sp, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                         int64_t* doc_chunk_offsets, int64_t* chunk_tokens, int64_t* chunk_bytes, int64_t* chunk_units, int64_t chunk_cap,
                         int64_t* needed_ids, int64_t* needed_chunks) {
    const int64_t n_docs = c.n_docs;
    c.out_cap = std::min<int64_t>(out_cap, c.total);
    const int64_t ccap = std::min<int64_t>(chunk_cap, c.total), cap = std::max<int64_t>(ccap, 1);      // (chunks <= tokens <= bytes: more capacity is never used)
    TKZ_TRY(stage_out(ws, n_docs, c.out_cap));
    HIP_TRY(ws->ck_stage.ensure((size_t)((n_docs + 1) + (cap + 1) + 2 * cap) * 8, &ws->bytes_allocated));
    int64_t* const d_dco = ws->ck_stage.as<int64_t>(), * const d_ct = d_dco + n_docs + 1, * const d_cb = d_ct + cap + 1, * const d_cu = d_cb + cap;
    c.d_out = ws->s_out[0].as<int32_t>(); c.d_out_offs = ws->s_outoffs[0].as<int64_t>();
    int64_t tokens = 0, chunks = 0;
    const tkz_status st = chunks_on_device(e, ws, c, ChunkCall{max_tokens, d_dco, d_ct, chunk_bytes ? d_cb : nullptr, chunk_units ? d_cu : nullptr, ccap, nullptr}, sp, &tokens, &chunks);
    if (needed_ids) *needed_ids = tokens;
    if (needed_chunks) *needed_chunks = chunks;
    if (st != TKZ_OK) return st;
    TKZ_TRY(fetch(ws, out_ids, tokens, out_offsets, n_docs));
    HIP_TRY(hipMemcpy(doc_chunk_offsets, d_dco, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(chunk_tokens, d_ct, (size_t)(chunks + 1) * 8, hipMemcpyDeviceToHost));
    if (chunk_bytes && chunks) HIP_TRY(hipMemcpy(chunk_bytes, d_cb, (size_t)chunks * 8, hipMemcpyDeviceToHost));
    if (chunk_units && chunks) HIP_TRY(hipMemcpy(chunk_units, d_cu, (size_t)chunks * 8, hipMemcpyDeviceToHost));
    return TKZ_OK;
}
const char* const kMsgChunkMax = "chunks: max_tokens must be at least 1";
const char* const kMsgChunkBufs = "chunks: null chunk table buffer or negative chunk_cap";
}  // namespace

tkz_status tkz_encode_batch_chunks_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                          const int32_t* allowed, int32_t n_allowed, int64_t max_tokens, int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets,
                                          int64_t* d_doc_chunk_offsets, int64_t* d_chunk_tokens, int64_t* d_chunk_bytes, int64_t* d_chunk_units, int64_t chunk_cap,
                                          void* hip_stream, int64_t* total_tokens, int64_t* n_chunks) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    if (max_tokens < 1) return fail(TKZ_E_ARG, kMsgChunkMax);
    if (!d_doc_chunk_offsets || !d_chunk_tokens || chunk_cap < 0) return fail(TKZ_E_ARG, kMsgChunkBufs);
    if (n_chunks) *n_chunks = 0;
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    DeviceScope scope;
    TKZ_TRY(check_device_call(e, scope, c));
    Lease lease(e);
    return chunks_on_device(e, lease.ws, c, ChunkCall{max_tokens, d_doc_chunk_offsets, d_chunk_tokens, d_chunk_bytes, d_chunk_units, chunk_cap, nullptr}, sp, total_tokens, n_chunks);
}

tkz_status tkz_encode_batch_chunks_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                        int64_t max_tokens, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* doc_chunk_offsets, int64_t* chunk_tokens,
                                        int64_t* chunk_bytes, int64_t* chunk_units, int64_t chunk_cap, int64_t* needed_ids, int64_t* needed_chunks) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    if (max_tokens < 1) return fail(TKZ_E_ARG, kMsgChunkMax);
    if (!doc_chunk_offsets || !chunk_tokens || chunk_cap < 0) return fail(TKZ_E_ARG, kMsgChunkBufs);
    TKZ_TRY(check_host_outputs(out_ids, out_cap, out_offsets, "null output buffer", false));
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(doc_offsets, n_docs, bytes != nullptr, kSizedDocs, &total));
    if (total == 0) TKZ_TRY(check_empty_docs(doc_offsets, n_docs, kSizedDocs, nullptr));      // (... and the device call runs all the same)
    if (needed_ids) *needed_ids = 0;
    if (needed_chunks) *needed_chunks = 0;
    // the whole batch is staged and the result copied from ONE call of the device entry, as tkz_encode_batch_spans_utf8 does
    Lease lease(e);
    Workspace* ws = lease.ws;
    TKZ_TRY(stage_in(ws, bytes, total, doc_offsets, n_docs));
    return chunks_staged(e, ws, staged_call(ws, n_docs, total, 0), max_tokens, sp, out_ids, out_cap, out_offsets, doc_chunk_offsets, chunk_tokens, chunk_bytes, chunk_units,
                         chunk_cap, needed_ids, needed_chunks);
}

// The same for UTF-16 documents: code units staged and transcoded on the device as tkz_encode_batch_spans_utf16 does; positions in code units only -- the bytes
// never exist on the host.
tkz_status tkz_encode_batch_chunks_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                         int64_t max_tokens, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int64_t* doc_chunk_offsets, int64_t* chunk_tokens,
                                         int64_t* chunk_units, int64_t chunk_cap, int64_t* needed_ids, int64_t* needed_chunks) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    if (max_tokens < 1) return fail(TKZ_E_ARG, kMsgChunkMax);
    if (!doc_chunk_offsets || !chunk_tokens || chunk_cap < 0) return fail(TKZ_E_ARG, kMsgChunkBufs);
    TKZ_TRY(check_host_outputs(out_ids, out_cap, out_offsets, "null output buffer", false));
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(unit_offsets, n_docs, units != nullptr, kUnitDocs, &total));
    if (needed_ids) *needed_ids = 0;
    if (needed_chunks) *needed_chunks = 0;
    if (total == 0) {
        TKZ_TRY(check_empty_docs(unit_offsets, n_docs, kUnitDocs, out_offsets));
        std::fill_n(doc_chunk_offsets, n_docs + 1, int64_t(0));
        chunk_tokens[0] = 0;
        ++e->chunks_calls;
        if (sp) ++e->spec_batches;
        return TKZ_OK;
    }
    Lease lease(e);
    Workspace* ws = lease.ws;
    U16Stage& U = ws->u16[0];
    const bool with_repl = sp && sp->fffd;
    HIP_TRY(U.ensure(total, n_docs, &ws->bytes_allocated, with_repl));
    HIP_TRY(hipMemcpy(U.units.p, units, (size_t)total * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U.offs.p, unit_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    const tkz::Launch L{nullptr, nullptr, ws};
    HIP_TRY(u16_measure(U, L, total, n_docs));
    HIP_TRY(hipStreamSynchronize(nullptr));
    int64_t nbytes = 0;                                                 // the batch as UTF-8
    TKZ_TRY(u16_write(U, L, total, n_docs, with_repl, &ws->bytes_allocated, &nbytes));
    BatchCall c{U.bytes.as<uint8_t>(), U.boffs.as<int64_t>(), n_docs, nbytes, nullptr, 0, nullptr, nullptr};
    if (with_repl) c.d_repl = U.repl.as<uint64_t>();
    return chunks_staged(e, ws, c, max_tokens, sp, out_ids, out_cap, out_offsets, doc_chunk_offsets, chunk_tokens, nullptr, chunk_units, chunk_cap, needed_ids, needed_chunks);
}

// ONE text: the batch entry with one document, at every size
tkz_status tkz_encode_chunks_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t max_tokens, int32_t* out_ids,
                                  int64_t out_cap, int64_t* chunk_tokens, int64_t* chunk_bytes, int64_t* chunk_units, int64_t chunk_cap, int64_t* n_out, int64_t* n_chunks) {
    if (len < 0 || !n_out || !n_chunks) return fail(TKZ_E_ARG, "bad argument");
    *n_out = 0; *n_chunks = 0;
    const int64_t offs[2] = {0, len};
    int64_t oo[2] = {0, 0}, dco[2] = {0, 0};
    return tkz_encode_batch_chunks_utf8(e, text, offs, 1, allowed, n_allowed, max_tokens, out_ids, out_cap, oo, dco, chunk_tokens, chunk_bytes, chunk_units, chunk_cap, n_out, n_chunks);
}
tkz_status tkz_encode_chunks_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t max_tokens, int32_t* out_ids,
                                   int64_t out_cap, int64_t* chunk_tokens, int64_t* chunk_units, int64_t chunk_cap, int64_t* n_out, int64_t* n_chunks) {
    if (len < 0 || (!text && len) || !n_out || !n_chunks) return fail(TKZ_E_ARG, "bad argument");
    *n_out = 0; *n_chunks = 0;
    const int64_t offs[2] = {0, len};
    int64_t oo[2] = {0, 0}, dco[2] = {0, 0};
    return tkz_encode_batch_chunks_utf16(e, text, offs, 1, allowed, n_allowed, max_tokens, out_ids, out_cap, oo, dco, chunk_tokens, chunk_units, chunk_cap, n_out, n_chunks);
}
void tkz_encoder_chunks_calls(const tkz_encoder* e, int64_t* calls) {
    if (calls) *calls = e ? e->chunks_calls.load() : 0;
}

// ---- overlapping token-budget chunks: the chunk entries with an overlap -- every chunk has a start AND an end in the table (tkz.h: the rule) ----

namespace {
const char* const kMsgChunkOverlap = "chunks: overlap must be in [0, max_tokens)";
const char* const kMsgChunkEnds = "chunks: null chunk table buffer (chunk_ends included) or negative chunk_cap";
tkz_status check_overlap_args(int64_t max_tokens, int64_t overlap, const void* doc_chunk_offsets, const void* chunk_tokens, const void* chunk_ends, int64_t chunk_cap) {
    if (max_tokens < 1) return fail(TKZ_E_ARG, kMsgChunkMax);
    if (overlap < 0 || overlap >= max_tokens) return fail(TKZ_E_ARG, kMsgChunkOverlap);
    if (!doc_chunk_offsets || !chunk_tokens || !chunk_ends || chunk_cap < 0) return fail(TKZ_E_ARG, kMsgChunkEnds);
    return TKZ_OK;
}
// where the host entries' table goes: chunk_tokens and chunk_ends, and the four position arrays (null: not asked for)
struct OverlapTable { int64_t* tokens; int64_t* ends; int64_t* pos[4]; };      // pos: chunk_bytes, chunk_units, chunk_end_bytes, chunk_end_units
// chunks_staged for the overlap entries: staging for the ids, their offsets and the six table arrays, ONE chunk call, the results back
tkz_status chunks_overlap_staged(tkz_encoder* e, Workspace* ws, BatchCall c, int64_t max_tokens, int64_t overlap, const SpecialCall* sp, int32_t* out_ids, int64_t out_cap,
                                 int64_t* out_offsets, int64_t* doc_chunk_offsets, const OverlapTable& t, int64_t chunk_cap, int64_t* needed_ids, int64_t* needed_chunks) {
    const int64_t n_docs = c.n_docs;
    c.out_cap = std::min<int64_t>(out_cap, c.total);
    const int64_t ccap = std::min<int64_t>(chunk_cap, c.total), cap = std::max<int64_t>(ccap, 1);      // (the starts ascend: chunks <= tokens <= bytes)
    TKZ_TRY(stage_out(ws, n_docs, c.out_cap));
    HIP_TRY(ws->ck_stage.ensure((size_t)((n_docs + 1) + 6 * cap) * 8, &ws->bytes_allocated));
    int64_t* const d_dco = ws->ck_stage.as<int64_t>(), * const d_ct = d_dco + n_docs + 1, * const d_ce = d_ct + cap, * const d_pos = d_ce + cap;
    c.d_out = ws->s_out[0].as<int32_t>(); c.d_out_offs = ws->s_outoffs[0].as<int64_t>();
    ChunkCall cc{max_tokens, d_dco, d_ct, t.pos[0] ? d_pos : nullptr, t.pos[1] ? d_pos + cap : nullptr, ccap, nullptr};
    cc.overlap = overlap; cc.d_chunk_ends = d_ce; cc.d_chunk_end_bytes = t.pos[2] ? d_pos + 2 * cap : nullptr; cc.d_chunk_end_units = t.pos[3] ? d_pos + 3 * cap : nullptr;
    int64_t tokens = 0, chunks = 0;
    const tkz_status st = chunks_on_device(e, ws, c, cc, sp, &tokens, &chunks);
    if (needed_ids) *needed_ids = tokens;
    if (needed_chunks) *needed_chunks = chunks;
    if (st != TKZ_OK) return st;
    TKZ_TRY(fetch(ws, out_ids, tokens, out_offsets, n_docs));
    HIP_TRY(hipMemcpy(doc_chunk_offsets, d_dco, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost));
    if (!chunks) return TKZ_OK;
    HIP_TRY(hipMemcpy(t.tokens, d_ct, (size_t)chunks * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t.ends, d_ce, (size_t)chunks * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; ++k) if (t.pos[k]) HIP_TRY(hipMemcpy(t.pos[k], d_pos + k * cap, (size_t)chunks * 8, hipMemcpyDeviceToHost));
    return TKZ_OK;
}
}  // namespace

tkz_status tkz_encode_batch_chunks_overlap_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                                  const int32_t* allowed, int32_t n_allowed, int64_t max_tokens, int64_t overlap, int32_t* d_out_ids, int64_t out_cap,
                                                  int64_t* d_out_offsets, int64_t* d_doc_chunk_offsets, int64_t* d_chunk_tokens, int64_t* d_chunk_ends,
                                                  int64_t* d_chunk_bytes, int64_t* d_chunk_units, int64_t* d_chunk_end_bytes, int64_t* d_chunk_end_units,
                                                  int64_t chunk_cap, void* hip_stream, int64_t* total_tokens, int64_t* n_chunks) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_overlap_args(max_tokens, overlap, d_doc_chunk_offsets, d_chunk_tokens, d_chunk_ends, chunk_cap));
    if (n_chunks) *n_chunks = 0;
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    DeviceScope scope;
    TKZ_TRY(check_device_call(e, scope, c));
    Lease lease(e);
    ChunkCall cc{max_tokens, d_doc_chunk_offsets, d_chunk_tokens, d_chunk_bytes, d_chunk_units, chunk_cap, nullptr};
    cc.overlap = overlap; cc.d_chunk_ends = d_chunk_ends; cc.d_chunk_end_bytes = d_chunk_end_bytes; cc.d_chunk_end_units = d_chunk_end_units;
    return chunks_on_device(e, lease.ws, c, cc, sp, total_tokens, n_chunks);
}

tkz_status tkz_encode_batch_chunks_overlap_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed,
                                                int32_t n_allowed, int64_t max_tokens, int64_t overlap, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                                int64_t* doc_chunk_offsets, int64_t* chunk_tokens, int64_t* chunk_ends, int64_t* chunk_bytes, int64_t* chunk_units,
                                                int64_t* chunk_end_bytes, int64_t* chunk_end_units, int64_t chunk_cap, int64_t* needed_ids, int64_t* needed_chunks) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_overlap_args(max_tokens, overlap, doc_chunk_offsets, chunk_tokens, chunk_ends, chunk_cap));
    TKZ_TRY(check_host_outputs(out_ids, out_cap, out_offsets, "null output buffer", false));
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(doc_offsets, n_docs, bytes != nullptr, kSizedDocs, &total));
    if (total == 0) TKZ_TRY(check_empty_docs(doc_offsets, n_docs, kSizedDocs, nullptr));      // (... and the device call runs all the same)
    if (needed_ids) *needed_ids = 0;
    if (needed_chunks) *needed_chunks = 0;
    Lease lease(e);
    Workspace* ws = lease.ws;
    TKZ_TRY(stage_in(ws, bytes, total, doc_offsets, n_docs));
    return chunks_overlap_staged(e, ws, staged_call(ws, n_docs, total, 0), max_tokens, overlap, sp, out_ids, out_cap, out_offsets, doc_chunk_offsets,
                                 OverlapTable{chunk_tokens, chunk_ends, {chunk_bytes, chunk_units, chunk_end_bytes, chunk_end_units}}, chunk_cap, needed_ids, needed_chunks);
}

// The same for UTF-16 documents, as tkz_encode_batch_chunks_utf16: positions in code units only
tkz_status tkz_encode_batch_chunks_overlap_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed,
                                                 int32_t n_allowed, int64_t max_tokens, int64_t overlap, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                                 int64_t* doc_chunk_offsets, int64_t* chunk_tokens, int64_t* chunk_ends, int64_t* chunk_units, int64_t* chunk_end_units,
                                                 int64_t chunk_cap, int64_t* needed_ids, int64_t* needed_chunks) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_overlap_args(max_tokens, overlap, doc_chunk_offsets, chunk_tokens, chunk_ends, chunk_cap));
    TKZ_TRY(check_host_outputs(out_ids, out_cap, out_offsets, "null output buffer", false));
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(unit_offsets, n_docs, units != nullptr, kUnitDocs, &total));
    if (needed_ids) *needed_ids = 0;
    if (needed_chunks) *needed_chunks = 0;
    if (total == 0) {
        TKZ_TRY(check_empty_docs(unit_offsets, n_docs, kUnitDocs, out_offsets));
        std::fill_n(doc_chunk_offsets, n_docs + 1, int64_t(0));
        ++e->chunks_overlap_calls;
        if (sp) ++e->spec_batches;
        return TKZ_OK;
    }
    Lease lease(e);
    Workspace* ws = lease.ws;
    U16Stage& U = ws->u16[0];
    const bool with_repl = sp && sp->fffd;
    HIP_TRY(U.ensure(total, n_docs, &ws->bytes_allocated, with_repl));
    HIP_TRY(hipMemcpy(U.units.p, units, (size_t)total * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U.offs.p, unit_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    const tkz::Launch L{nullptr, nullptr, ws};
    HIP_TRY(u16_measure(U, L, total, n_docs));
    HIP_TRY(hipStreamSynchronize(nullptr));
    int64_t nbytes = 0;                                                 // the batch as UTF-8
    TKZ_TRY(u16_write(U, L, total, n_docs, with_repl, &ws->bytes_allocated, &nbytes));
    BatchCall c{U.bytes.as<uint8_t>(), U.boffs.as<int64_t>(), n_docs, nbytes, nullptr, 0, nullptr, nullptr};
    if (with_repl) c.d_repl = U.repl.as<uint64_t>();
    return chunks_overlap_staged(e, ws, c, max_tokens, overlap, sp, out_ids, out_cap, out_offsets, doc_chunk_offsets,
                                 OverlapTable{chunk_tokens, chunk_ends, {nullptr, chunk_units, nullptr, chunk_end_units}}, chunk_cap, needed_ids, needed_chunks);
}

// ONE text: the batch entry with one document, at every size
tkz_status tkz_encode_chunks_overlap_utf8(tkz_encoder* e, const uint8_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t max_tokens,
                                          int64_t overlap, int32_t* out_ids, int64_t out_cap, int64_t* chunk_tokens, int64_t* chunk_ends, int64_t* chunk_bytes,
                                          int64_t* chunk_units, int64_t* chunk_end_bytes, int64_t* chunk_end_units, int64_t chunk_cap, int64_t* n_out, int64_t* n_chunks) {
    if (len < 0 || !n_out || !n_chunks) return fail(TKZ_E_ARG, "bad argument");
    *n_out = 0; *n_chunks = 0;
    const int64_t offs[2] = {0, len};
    int64_t oo[2] = {0, 0}, dco[2] = {0, 0};
    return tkz_encode_batch_chunks_overlap_utf8(e, text, offs, 1, allowed, n_allowed, max_tokens, overlap, out_ids, out_cap, oo, dco, chunk_tokens, chunk_ends, chunk_bytes,
                                                chunk_units, chunk_end_bytes, chunk_end_units, chunk_cap, n_out, n_chunks);
}
tkz_status tkz_encode_chunks_overlap_utf16(tkz_encoder* e, const uint16_t* text, int64_t len, const int32_t* allowed, int32_t n_allowed, int64_t max_tokens,
                                           int64_t overlap, int32_t* out_ids, int64_t out_cap, int64_t* chunk_tokens, int64_t* chunk_ends, int64_t* chunk_units,
                                           int64_t* chunk_end_units, int64_t chunk_cap, int64_t* n_out, int64_t* n_chunks) {
    if (len < 0 || (!text && len) || !n_out || !n_chunks) return fail(TKZ_E_ARG, "bad argument");
    *n_out = 0; *n_chunks = 0;
    const int64_t offs[2] = {0, len};
    int64_t oo[2] = {0, 0}, dco[2] = {0, 0};
    return tkz_encode_batch_chunks_overlap_utf16(e, text, offs, 1, allowed, n_allowed, max_tokens, overlap, out_ids, out_cap, oo, dco, chunk_tokens, chunk_ends, chunk_units,
                                                 chunk_end_units, chunk_cap, n_out, n_chunks);
}
void tkz_encoder_chunks_overlap_calls(const tkz_encoder* e, int64_t* calls) {
    if (calls) *calls = e ? e->chunks_overlap_calls.load() : 0;
}

// ---- packed rows: the ids of the matching encode entry framed by bos / eos ids, laid out in rows of row_len, with pos and seg_starts (tkz.h: the rule) ----

namespace {
tkz_status check_pack_args(int32_t bos_id, int32_t eos_id, int64_t row_len, const void* seg_starts, int64_t seg_cap) {
    if (bos_id < -1 || eos_id < -1) return fail(TKZ_E_ARG, "packed rows: bos_id and eos_id are -1 (none) or an id >= 0");
    if (row_len < 1 || row_len > (int64_t)INT32_MAX) return fail(TKZ_E_ARG, "packed rows: row_len must be in [1, 2^31 - 1]");
    if (seg_starts && seg_cap < 0) return fail(TKZ_E_ARG, "packed rows: negative seg_cap");
    return TKZ_OK;
}
// the packed call on device buffers, on a workspace the entry holds: the plain launch sequence -- with the unframed ids and offsets in the workspace when the
// documents are framed --, then the rows (enqueue_attempt)
tkz_status packed_on_device(tkz_encoder* e, Workspace* ws, BatchCall c, PackCall pc, const SpecialCall* sp, int64_t* total_tokens, int64_t* n_rows, int64_t* n_segs) {
    int64_t* acc = &ws->bytes_allocated;
    const int64_t ntile = pack_tiles(c.total, c.n_docs, pc);
    if (pc.frame() > 0) {
        if (c.total > 0) HIP_TRY(ws->pk_ids.ensure((size_t)c.total * 4, acc));
        HIP_TRY(ws->pk_offs.ensure((size_t)(c.n_docs + 1) * 8, acc));
    }
    HIP_TRY(ws->pk_cnt.ensure((size_t)std::max<int64_t>(ntile, 1) * 4, acc));
    HIP_TRY(ws->pk_base.ensure((size_t)(ntile + 1) * 8, acc));
    HIP_TRY(ws->pk_bsum.ensure((size_t)(ntile / tkz::kScanBlock + 2) * 8, acc));
    int64_t rows = 0, segs = 0;
    pc.n_rows = &rows; pc.n_segs = &segs;
    c.kind = CallKind::Packed; c.packed = &pc; c.special = sp;
    const tkz_status st = encode_device(e, ws, c, kCallWhole, total_tokens);
    if (n_rows) *n_rows = rows;
    if (n_segs) *n_segs = segs;
    if (st == TKZ_OK) { ++e->packed_calls; if (sp) ++e->spec_batches; }
    return st;
}
// The second half of a packed host entry, with the batch on the device as UTF-8 (c: its bytes and byte offsets): staging for the rows, the offsets, pos and
// seg_starts, ONE packed call, the results back.
tkz_status packed_staged(tkz_encoder* e, Workspace* ws, BatchCall c, int32_t bos_id, int32_t eos_id, int64_t row_len, int32_t pad_id, const SpecialCall* sp,
                         int32_t* out_ids, int64_t out_cap, int64_t* out_offsets, int32_t* pos, int64_t* seg_starts, int64_t seg_cap,
                         int64_t* total_tokens, int64_t* needed_ids, int64_t* needed_segs) {
    const int64_t n_docs = c.n_docs;
    const PackCall frame{bos_id, eos_id, row_len, pad_id, nullptr, nullptr, 0, nullptr, nullptr};
    const int64_t rows_bound = (c.total + frame.frame() * n_docs + row_len - 1) / row_len;      // (tokens <= bytes: more capacity is never used)
    c.out_cap = std::min<int64_t>(out_cap, rows_bound * row_len);
    const int64_t cap = std::max<int64_t>(c.out_cap, 1), scap = seg_starts ? std::min<int64_t>(seg_cap, n_docs + rows_bound) : 0;
    TKZ_TRY(stage_out(ws, n_docs, c.out_cap));
    HIP_TRY(ws->pk_stage.ensure((size_t)(scap + 1) * 8 + (size_t)cap * 4, &ws->bytes_allocated));
    int64_t* const d_seg = ws->pk_stage.as<int64_t>();
    int32_t* const d_pos = reinterpret_cast<int32_t*>(d_seg + scap + 1);
    c.d_out = ws->s_out[0].as<int32_t>(); c.d_out_offs = ws->s_outoffs[0].as<int64_t>();
    int64_t tokens = 0, rows = 0, segs = 0;
    const tkz_status st = packed_on_device(e, ws, c, PackCall{bos_id, eos_id, row_len, pad_id, pos ? d_pos : nullptr, seg_starts ? d_seg : nullptr, scap, nullptr, nullptr}, sp,
                                           &tokens, &rows, &segs);
    if (total_tokens) *total_tokens = tokens;
    *needed_ids = rows * row_len; *needed_segs = segs;
    if (st != TKZ_OK) return st;
    TKZ_TRY(fetch(ws, out_ids, rows * row_len, out_offsets, n_docs));
    if (pos && rows) HIP_TRY(hipMemcpy(pos, d_pos, (size_t)(rows * row_len) * 4, hipMemcpyDeviceToHost));
    if (seg_starts) HIP_TRY(hipMemcpy(seg_starts, d_seg, (size_t)(segs + 1) * 8, hipMemcpyDeviceToHost));
    return TKZ_OK;
}
const char* const kMsgPackCounts = "packed rows: null count pointer";
}  // namespace

tkz_status tkz_encode_batch_packed_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                          const int32_t* allowed, int32_t n_allowed, int32_t bos_id, int32_t eos_id, int64_t row_len, int32_t pad_id,
                                          int32_t* d_out_ids, int64_t out_cap, int64_t* d_out_offsets, int32_t* d_pos, int64_t* d_seg_starts, int64_t seg_cap,
                                          void* hip_stream, int64_t* total_tokens, int64_t* n_rows, int64_t* n_segs) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pack_args(bos_id, eos_id, row_len, d_seg_starts, seg_cap));
    if (!total_tokens || !n_rows || !n_segs) return fail(TKZ_E_ARG, kMsgPackCounts);
    *total_tokens = 0; *n_rows = 0; *n_segs = 0;
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    DeviceScope scope;
    TKZ_TRY(check_device_call(e, scope, c));
    if (out_cap > 0 && !d_out_ids) return fail(TKZ_E_ARG, "null device buffer");      // (a batch without bytes still has a stream when it is framed)
    Lease lease(e);
    return packed_on_device(e, lease.ws, c, PackCall{bos_id, eos_id, row_len, pad_id, d_pos, d_seg_starts, seg_cap, nullptr, nullptr}, sp, total_tokens, n_rows, n_segs);
}

tkz_status tkz_encode_batch_packed_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                        int32_t bos_id, int32_t eos_id, int64_t row_len, int32_t pad_id, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                        int32_t* pos, int64_t* seg_starts, int64_t seg_cap, int64_t* total_tokens, int64_t* needed_ids, int64_t* needed_segs) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pack_args(bos_id, eos_id, row_len, seg_starts, seg_cap));
    if (!needed_ids || !needed_segs) return fail(TKZ_E_ARG, kMsgPackCounts);
    TKZ_TRY(check_host_outputs(out_ids, out_cap, out_offsets, "null output buffer", false));
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(doc_offsets, n_docs, bytes != nullptr, kSizedDocs, &total));
    if (total == 0) TKZ_TRY(check_empty_docs(doc_offsets, n_docs, kSizedDocs, nullptr));      // (... and the device call runs all the same)
    if (total_tokens) *total_tokens = 0;
    *needed_ids = 0; *needed_segs = 0;
    // the whole batch is staged and the result copied from ONE call of the device entry, as tkz_encode_batch_spans_utf8 does
    Lease lease(e);
    Workspace* ws = lease.ws;
    TKZ_TRY(stage_in(ws, bytes, total, doc_offsets, n_docs));
    return packed_staged(e, ws, staged_call(ws, n_docs, total, 0), bos_id, eos_id, row_len, pad_id, sp, out_ids, out_cap, out_offsets, pos, seg_starts, seg_cap,
                         total_tokens, needed_ids, needed_segs);
}

// The same for UTF-16 documents: code units staged and transcoded on the device as tkz_encode_batch_spans_utf16 does.
tkz_status tkz_encode_batch_packed_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                         int32_t bos_id, int32_t eos_id, int64_t row_len, int32_t pad_id, int32_t* out_ids, int64_t out_cap, int64_t* out_offsets,
                                         int32_t* pos, int64_t* seg_starts, int64_t seg_cap, int64_t* total_tokens, int64_t* needed_ids, int64_t* needed_segs) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pack_args(bos_id, eos_id, row_len, seg_starts, seg_cap));
    if (!needed_ids || !needed_segs) return fail(TKZ_E_ARG, kMsgPackCounts);
    TKZ_TRY(check_host_outputs(out_ids, out_cap, out_offsets, "null output buffer", false));
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(unit_offsets, n_docs, units != nullptr, kUnitDocs, &total));
    if (total_tokens) *total_tokens = 0;
    *needed_ids = 0; *needed_segs = 0;
    Lease lease(e);
    Workspace* ws = lease.ws;
    if (total == 0) {                                                   // (no units: the offsets, all 0, are byte offsets as they are -- the framing is still laid out)
        TKZ_TRY(check_empty_docs(unit_offsets, n_docs, kUnitDocs, nullptr));
        TKZ_TRY(stage_in(ws, nullptr, 0, unit_offsets, n_docs));
        return packed_staged(e, ws, staged_call(ws, n_docs, 0, 0), bos_id, eos_id, row_len, pad_id, sp, out_ids, out_cap, out_offsets, pos, seg_starts, seg_cap,
                             total_tokens, needed_ids, needed_segs);
    }
    U16Stage& U = ws->u16[0];
    const bool with_repl = sp && sp->fffd;
    HIP_TRY(U.ensure(total, n_docs, &ws->bytes_allocated, with_repl));
    HIP_TRY(hipMemcpy(U.units.p, units, (size_t)total * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U.offs.p, unit_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    const tkz::Launch L{nullptr, nullptr, ws};
    HIP_TRY(u16_measure(U, L, total, n_docs));
    HIP_TRY(hipStreamSynchronize(nullptr));
    int64_t nbytes = 0;                                                 // the batch as UTF-8
    TKZ_TRY(u16_write(U, L, total, n_docs, with_repl, &ws->bytes_allocated, &nbytes));
    BatchCall c{U.bytes.as<uint8_t>(), U.boffs.as<int64_t>(), n_docs, nbytes, nullptr, 0, nullptr, nullptr};
    if (with_repl) c.d_repl = U.repl.as<uint64_t>();
    return packed_staged(e, ws, c, bos_id, eos_id, row_len, pad_id, sp, out_ids, out_cap, out_offsets, pos, seg_starts, seg_cap, total_tokens, needed_ids, needed_segs);
}
void tkz_encoder_packed_calls(const tkz_encoder* e, int64_t* calls) {
    if (calls) *calls = e ? e->packed_calls.load() : 0;
}

// ---- padded rows: the ids of the matching encode entry cut to max_len, framed by bos / eos ids, a row a document padded to the common width (tkz.h: the rule) ----

namespace {
tkz_status check_pad_args(int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int64_t pad_multiple) {
    if (bos_id < -1 || eos_id < -1) return fail(TKZ_E_ARG, "padded rows: bos_id and eos_id are -1 (none) or an id >= 0");
    const int64_t f = (bos_id >= 0) + (eos_id >= 0);
    if (max_len < std::max<int64_t>(1, f) || max_len > (int64_t)INT32_MAX) return fail(TKZ_E_ARG, "padded rows: max_len must be in [max(1, framing ids), 2^31 - 1]");
    if (cut_side != TKZ_TRIM_SUFFIX && cut_side != TKZ_TRIM_PREFIX) return fail(TKZ_E_ARG, "padded rows: cut_side must be TKZ_TRIM_SUFFIX or TKZ_TRIM_PREFIX");
    if (pad_side != TKZ_PAD_RIGHT && pad_side != TKZ_PAD_LEFT) return fail(TKZ_E_ARG, "padded rows: pad_side must be TKZ_PAD_RIGHT or TKZ_PAD_LEFT");
    if (pad_multiple < 0 || pad_multiple > (int64_t)INT32_MAX) return fail(TKZ_E_ARG, "padded rows: pad_multiple must be in [0, 2^31 - 1]");
    return TKZ_OK;
}
const char* const kMsgPadPointers = "padded rows: null ids, lens or scalar pointer";
// the padded call on device buffers, on a workspace the entry holds: the plain launch sequence with the uncut ids and offsets in the workspace, then the rows
// (enqueue_attempt)
tkz_status padded_on_device(tkz_encoder* e, Workspace* ws, BatchCall c, PadCall pc, const SpecialCall* sp, int64_t* total_tokens, int64_t* width, int64_t* n_cut) {
    int64_t* acc = &ws->bytes_allocated;
    if (c.n_docs < 0 || c.total < 0 || c.out_cap < 0) return fail(TKZ_E_ARG, "negative size");
    if (c.total > 0) HIP_TRY(ws->pd_ids.ensure((size_t)c.total * 4, acc));
    HIP_TRY(ws->pd_offs.ensure((size_t)(c.n_docs + 1) * 8, acc));
    HIP_TRY(ws->pd_src.ensure((size_t)std::max<int64_t>(c.n_docs, 1) * 8, acc));
    HIP_TRY(ws->pd_part.ensure((size_t)tkz::kPadGridMax * 12, acc));
    int64_t w = 0, cut = 0;
    pc.width = &w; pc.n_cut = &cut;
    c.kind = CallKind::Padded; c.padded = &pc; c.special = sp;
    const tkz_status st = encode_device(e, ws, c, kCallWhole, total_tokens);
    if (width) *width = w;
    if (n_cut) *n_cut = cut;
    if (st == TKZ_OK) { ++e->padded_calls; if (sp) ++e->spec_batches; }
    return st;
}
// The second half of a padded host entry, with the batch on the device as UTF-8 (c: its bytes and byte offsets): staging for the rows, the offsets, pos, lens and
// the mask, ONE padded call, the results back -- n_docs * W entries of each, never the uncut ids.
tkz_status padded_staged(tkz_encoder* e, Workspace* ws, BatchCall c, PadCall pc, const SpecialCall* sp, int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos,
                         int32_t* lens, int64_t* out_offsets, int64_t* total_tokens, int64_t* width, int64_t* n_cut) {
    const int64_t n_docs = c.n_docs;
    const bool fits = n_docs == 0 || out_cap / pc.max_len >= n_docs;      // (n_docs * max_len always suffices: more capacity is never used)
    c.out_cap = fits ? n_docs * pc.max_len : out_cap;
    const int64_t cap = std::max<int64_t>(c.out_cap, 1), nl = std::max<int64_t>(n_docs, 1);
    TKZ_TRY(stage_out(ws, n_docs, c.out_cap, out_offsets != nullptr));
    HIP_TRY(ws->pd_stage.ensure((size_t)(pos ? cap : 0) * 4 + (size_t)nl * 4 + (size_t)(mask ? cap : 0), &ws->bytes_allocated));
    int32_t* const d_pos = ws->pd_stage.as<int32_t>();
    int32_t* const d_lens = d_pos + (pos ? cap : 0);
    uint8_t* const d_mask = reinterpret_cast<uint8_t*>(d_lens + nl);
    c.d_out = ws->s_out[0].as<int32_t>(); c.d_out_offs = out_offsets ? ws->s_outoffs[0].as<int64_t>() : nullptr;
    pc.d_mask = mask ? d_mask : nullptr; pc.d_pos = pos ? d_pos : nullptr; pc.d_lens = d_lens;
    const tkz_status st = padded_on_device(e, ws, c, pc, sp, total_tokens, width, n_cut);
    if (st != TKZ_OK) return st;
    const int64_t n = n_docs * *width;
    TKZ_TRY(fetch(ws, out_ids, n, out_offsets, n_docs));
    if (n_docs) HIP_TRY(hipMemcpy(lens, d_lens, (size_t)n_docs * 4, hipMemcpyDeviceToHost));
    if (pos && n) HIP_TRY(hipMemcpy(pos, d_pos, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (mask && n) HIP_TRY(hipMemcpy(mask, d_mask, (size_t)n, hipMemcpyDeviceToHost));
    return TKZ_OK;
}
}  // namespace

tkz_status tkz_encode_batch_padded_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                          const int32_t* allowed, int32_t n_allowed, int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side,
                                          int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int32_t* d_out_ids, int64_t out_cap, uint8_t* d_mask,
                                          int32_t* d_pos, int32_t* d_lens, int64_t* d_out_offsets, void* hip_stream, int64_t* total_tokens, int64_t* width,
                                          int64_t* n_cut) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pad_args(bos_id, eos_id, max_len, cut_side, pad_side, pad_multiple));
    if (!d_out_ids || !d_lens || !total_tokens || !width || !n_cut) return fail(TKZ_E_ARG, kMsgPadPointers);
    *total_tokens = 0; *width = 0; *n_cut = 0;
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    if (!d_doc_offsets || (total_bytes > 0 && !d_bytes)) return fail(TKZ_E_ARG, "null device buffer");      // (d_out_offsets may be null here)
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(TKZ_E_ARG, "d_bytes must be 16-byte aligned");
    Lease lease(e);
    return padded_on_device(e, lease.ws, c, PadCall{bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, d_mask, d_pos, d_lens, nullptr, nullptr}, sp,
                            total_tokens, width, n_cut);
}

tkz_status tkz_encode_batch_padded_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                        int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                        int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos, int32_t* lens, int64_t* out_offsets,
                                        int64_t* total_tokens, int64_t* width, int64_t* n_cut) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pad_args(bos_id, eos_id, max_len, cut_side, pad_side, pad_multiple));
    if (!out_ids || !lens || !total_tokens || !width || !n_cut || out_cap < 0) return fail(TKZ_E_ARG, kMsgPadPointers);
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(doc_offsets, n_docs, bytes != nullptr, kSizedDocs, &total));
    if (total == 0) TKZ_TRY(check_empty_docs(doc_offsets, n_docs, kSizedDocs, nullptr));      // (... and the device call runs all the same)
    *total_tokens = 0; *width = 0; *n_cut = 0;
    // the whole batch is staged and the result copied from ONE call of the device entry, as tkz_encode_batch_packed_utf8 does
    Lease lease(e);
    Workspace* ws = lease.ws;
    TKZ_TRY(stage_in(ws, bytes, total, doc_offsets, n_docs));
    return padded_staged(e, ws, staged_call(ws, n_docs, total, 0), PadCall{bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, nullptr, nullptr, nullptr, nullptr, nullptr},
                         sp, out_ids, out_cap, mask, pos, lens, out_offsets, total_tokens, width, n_cut);
}

// The same for UTF-16 documents: code units staged and transcoded on the device as tkz_encode_batch_packed_utf16 does.
tkz_status tkz_encode_batch_padded_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                         int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                         int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos, int32_t* lens, int64_t* out_offsets,
                                         int64_t* total_tokens, int64_t* width, int64_t* n_cut) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pad_args(bos_id, eos_id, max_len, cut_side, pad_side, pad_multiple));
    if (!out_ids || !lens || !total_tokens || !width || !n_cut || out_cap < 0) return fail(TKZ_E_ARG, kMsgPadPointers);
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(unit_offsets, n_docs, units != nullptr, kUnitDocs, &total));
    *total_tokens = 0; *width = 0; *n_cut = 0;
    const PadCall pc{bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, nullptr, nullptr, nullptr, nullptr, nullptr};
    Lease lease(e);
    Workspace* ws = lease.ws;
    if (total == 0) {                                                   // (no units: the offsets, all 0, are byte offsets as they are -- the framing is still laid out)
        TKZ_TRY(check_empty_docs(unit_offsets, n_docs, kUnitDocs, nullptr));
        TKZ_TRY(stage_in(ws, nullptr, 0, unit_offsets, n_docs));
        return padded_staged(e, ws, staged_call(ws, n_docs, 0, 0), pc, sp, out_ids, out_cap, mask, pos, lens, out_offsets, total_tokens, width, n_cut);
    }
    U16Stage& U = ws->u16[0];
    const bool with_repl = sp && sp->fffd;
    HIP_TRY(U.ensure(total, n_docs, &ws->bytes_allocated, with_repl));
    HIP_TRY(hipMemcpy(U.units.p, units, (size_t)total * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U.offs.p, unit_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    const tkz::Launch L{nullptr, nullptr, ws};
    HIP_TRY(u16_measure(U, L, total, n_docs));
    HIP_TRY(hipStreamSynchronize(nullptr));
    int64_t nbytes = 0;                                                 // the batch as UTF-8
    TKZ_TRY(u16_write(U, L, total, n_docs, with_repl, &ws->bytes_allocated, &nbytes));
    BatchCall c{U.bytes.as<uint8_t>(), U.boffs.as<int64_t>(), n_docs, nbytes, nullptr, 0, nullptr, nullptr};
    if (with_repl) c.d_repl = U.repl.as<uint64_t>();
    return padded_staged(e, ws, c, pc, sp, out_ids, out_cap, mask, pos, lens, out_offsets, total_tokens, width, n_cut);
}
void tkz_encoder_padded_calls(const tkz_encoder* e, int64_t* calls) {
    if (calls) *calls = e ? e->padded_calls.load() : 0;
}

// ---- length-bucketed padded rows: the padded rows of the documents sorted by length, every bucket of bucket_rows rows at its own width (tkz.h: the rule) ----

namespace {
tkz_status check_bkt_args(int64_t bucket_rows, int32_t order) {
    if (bucket_rows < 1 || bucket_rows > (int64_t)INT32_MAX) return fail(TKZ_E_ARG, "bucketed rows: bucket_rows must be in [1, 2^31 - 1]");
    if (order != TKZ_BUCKET_ASCENDING && order != TKZ_BUCKET_DESCENDING) return fail(TKZ_E_ARG, "bucketed rows: order must be TKZ_BUCKET_ASCENDING or TKZ_BUCKET_DESCENDING");
    return TKZ_OK;
}
const char* const kMsgBktPointers = "bucketed rows: null ids, lens, order, bucket table or scalar pointer";
// the bucketed call on device buffers, on a workspace the entry holds: the padded call's sequence with the sort, the table and the rows behind k_pad_lens
tkz_status bucketed_on_device(tkz_encoder* e, Workspace* ws, BatchCall c, PadCall pc, BktCall bc, const SpecialCall* sp, int64_t* total_tokens, int64_t* total_positions,
                              int64_t* n_cut) {
    int64_t* acc = &ws->bytes_allocated;
    if (c.n_docs < 0 || c.total < 0 || c.out_cap < 0) return fail(TKZ_E_ARG, "negative size");
    const int64_t n = std::max<int64_t>(c.n_docs, 1), nt = tkz::bkt_sort_tiles(c.n_docs), nb = bc.buckets(c.n_docs);
    if (c.total > 0) HIP_TRY(ws->pd_ids.ensure((size_t)c.total * 4, acc));
    HIP_TRY(ws->pd_offs.ensure((size_t)(c.n_docs + 1) * 8, acc));
    HIP_TRY(ws->pd_src.ensure((size_t)n * 8, acc));
    HIP_TRY(ws->pd_part.ensure((size_t)tkz::kPadGridMax * 12, acc));
    HIP_TRY(ws->bk_keys.ensure((size_t)n * 3 * 4, acc));      // (key_a, key_b, slen)
    HIP_TRY(ws->bk_idx.ensure((size_t)n * 3 * 8, acc));       // (idx_a, idx_b, ssrc)
    HIP_TRY(ws->bk_hist.ensure((size_t)nt * 256 * 4, acc));
    HIP_TRY(ws->bk_base.ensure((size_t)(nt * 256 + 1) * 8, acc));
    HIP_TRY(ws->bk_bsum.ensure((size_t)(std::max(nt * 256, nb) / tkz::kScanBlock + 2) * 8, acc));
    HIP_TRY(ws->bk_cnt.ensure((size_t)std::max<int64_t>(nb, 1) * 8, acc));
    HIP_TRY(ws->bk_boffs.ensure((size_t)(nb + 1) * 8, acc));
    int64_t p = 0, cut = 0;
    pc.width = &p; pc.n_cut = &cut;
    c.kind = CallKind::Bucketed; c.padded = &pc; c.bucketed = &bc; c.special = sp;
    const tkz_status st = encode_device(e, ws, c, kCallWhole, total_tokens);
    if (total_positions) *total_positions = p;
    if (n_cut) *n_cut = cut;
    if (st == TKZ_OK) { ++e->bucketed_calls; if (sp) ++e->spec_batches; }
    return st;
}
// The second half of a bucketed host entry, with the batch on the device as UTF-8: staging for the rows (n_docs * max_len positions at most), the offsets, pos,
// lens, the mask, order, rank and the bucket table, ONE bucketed call, the results back -- P entries of the rows, never the uncut ids.
tkz_status bucketed_staged(tkz_encoder* e, Workspace* ws, BatchCall c, PadCall pc, BktCall bc, const SpecialCall* sp, int32_t* out_ids, int64_t out_cap, uint8_t* mask,
                           int32_t* pos, int32_t* lens, int64_t* out_offsets, int64_t* order, int64_t* rank, int64_t* bucket_offsets, int32_t* bucket_widths,
                           int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut) {
    const int64_t n_docs = c.n_docs, nb = bc.buckets(n_docs);
    const bool fits = n_docs == 0 || out_cap / pc.max_len >= n_docs;      // (n_docs * max_len always suffices: more capacity is never used)
    c.out_cap = fits ? n_docs * pc.max_len : out_cap;
    const int64_t cap = std::max<int64_t>(c.out_cap, 1), nl = std::max<int64_t>(n_docs, 1);
    TKZ_TRY(stage_out(ws, n_docs, c.out_cap, out_offsets != nullptr));
    HIP_TRY(ws->pd_stage.ensure((size_t)(pos ? cap : 0) * 4 + (size_t)nl * 4 + (size_t)(mask ? cap : 0), &ws->bytes_allocated));
    HIP_TRY(ws->bk_stage.ensure((size_t)nl * 16 + (size_t)(nb + 1) * 8 + (size_t)(nb + 1) * 4, &ws->bytes_allocated));
    int32_t* const d_pos = ws->pd_stage.as<int32_t>();
    int32_t* const d_lens = d_pos + (pos ? cap : 0);
    uint8_t* const d_mask = reinterpret_cast<uint8_t*>(d_lens + nl);
    int64_t* const d_order = ws->bk_stage.as<int64_t>();
    int64_t* const d_rank = d_order + nl;
    int64_t* const d_boffs = d_rank + nl;
    int32_t* const d_widths = reinterpret_cast<int32_t*>(d_boffs + nb + 1);
    c.d_out = ws->s_out[0].as<int32_t>(); c.d_out_offs = out_offsets ? ws->s_outoffs[0].as<int64_t>() : nullptr;
    pc.d_mask = mask ? d_mask : nullptr; pc.d_pos = pos ? d_pos : nullptr; pc.d_lens = d_lens;
    bc.d_order = d_order; bc.d_rank = rank ? d_rank : nullptr; bc.d_bucket_offs = d_boffs; bc.d_bucket_widths = d_widths;
    const tkz_status st = bucketed_on_device(e, ws, c, pc, bc, sp, total_tokens, total_positions, n_cut);
    if (st != TKZ_OK) return st;
    const int64_t n = *total_positions;
    TKZ_TRY(fetch(ws, out_ids, n, out_offsets, n_docs));
    HIP_TRY(hipMemcpy(bucket_offsets, d_boffs, (size_t)(nb + 1) * 8, hipMemcpyDeviceToHost));
    if (n_docs) {
        HIP_TRY(hipMemcpy(lens, d_lens, (size_t)n_docs * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(order, d_order, (size_t)n_docs * 8, hipMemcpyDeviceToHost));
        if (rank) HIP_TRY(hipMemcpy(rank, d_rank, (size_t)n_docs * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(bucket_widths, d_widths, (size_t)nb * 4, hipMemcpyDeviceToHost));
    }
    if (pos && n) HIP_TRY(hipMemcpy(pos, d_pos, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (mask && n) HIP_TRY(hipMemcpy(mask, d_mask, (size_t)n, hipMemcpyDeviceToHost));
    return TKZ_OK;
}
}  // namespace

tkz_status tkz_encode_batch_bucketed_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                            const int32_t* allowed, int32_t n_allowed, int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side,
                                            int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int64_t bucket_rows, int32_t order, int32_t* d_out_ids,
                                            int64_t out_cap, uint8_t* d_mask, int32_t* d_pos, int32_t* d_lens, int64_t* d_out_offsets, int64_t* d_order,
                                            int64_t* d_rank, int64_t* d_bucket_offsets, int32_t* d_bucket_widths, void* hip_stream, int64_t* total_tokens,
                                            int64_t* total_positions, int64_t* n_cut) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pad_args(bos_id, eos_id, max_len, cut_side, pad_side, pad_multiple));
    TKZ_TRY(check_bkt_args(bucket_rows, order));
    if (!d_out_ids || !d_lens || !d_order || !d_bucket_offsets || !d_bucket_widths || !total_tokens || !total_positions || !n_cut) return fail(TKZ_E_ARG, kMsgBktPointers);
    *total_tokens = 0; *total_positions = 0; *n_cut = 0;
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    if (!d_doc_offsets || (total_bytes > 0 && !d_bytes)) return fail(TKZ_E_ARG, "null device buffer");      // (d_out_offsets may be null here)
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(TKZ_E_ARG, "d_bytes must be 16-byte aligned");
    Lease lease(e);
    return bucketed_on_device(e, lease.ws, c, PadCall{bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, d_mask, d_pos, d_lens, nullptr, nullptr},
                              BktCall{bucket_rows, order, d_order, d_rank, d_bucket_offsets, d_bucket_widths}, sp, total_tokens, total_positions, n_cut);
}

tkz_status tkz_encode_batch_bucketed_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                          int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                          int64_t bucket_rows, int32_t order, int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos, int32_t* lens,
                                          int64_t* out_offsets, int64_t* order_out, int64_t* rank, int64_t* bucket_offsets, int32_t* bucket_widths,
                                          int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pad_args(bos_id, eos_id, max_len, cut_side, pad_side, pad_multiple));
    TKZ_TRY(check_bkt_args(bucket_rows, order));
    if (!out_ids || !lens || !order_out || !bucket_offsets || !bucket_widths || !total_tokens || !total_positions || !n_cut || out_cap < 0) return fail(TKZ_E_ARG, kMsgBktPointers);
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(doc_offsets, n_docs, bytes != nullptr, kSizedDocs, &total));
    if (total == 0) TKZ_TRY(check_empty_docs(doc_offsets, n_docs, kSizedDocs, nullptr));      // (... and the device call runs all the same)
    *total_tokens = 0; *total_positions = 0; *n_cut = 0;
    // the whole batch is staged and the result copied from ONE call of the device entry, as tkz_encode_batch_padded_utf8 does
    Lease lease(e);
    Workspace* ws = lease.ws;
    TKZ_TRY(stage_in(ws, bytes, total, doc_offsets, n_docs));
    return bucketed_staged(e, ws, staged_call(ws, n_docs, total, 0), PadCall{bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, nullptr, nullptr, nullptr, nullptr, nullptr},
                           BktCall{bucket_rows, order, nullptr, nullptr, nullptr, nullptr}, sp, out_ids, out_cap, mask, pos, lens, out_offsets, order_out, rank, bucket_offsets,
                           bucket_widths, total_tokens, total_positions, n_cut);
}

// The same for UTF-16 documents: code units staged and transcoded on the device as tkz_encode_batch_padded_utf16 does.
tkz_status tkz_encode_batch_bucketed_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                           int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                           int64_t bucket_rows, int32_t order, int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos, int32_t* lens,
                                           int64_t* out_offsets, int64_t* order_out, int64_t* rank, int64_t* bucket_offsets, int32_t* bucket_widths,
                                           int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pad_args(bos_id, eos_id, max_len, cut_side, pad_side, pad_multiple));
    TKZ_TRY(check_bkt_args(bucket_rows, order));
    if (!out_ids || !lens || !order_out || !bucket_offsets || !bucket_widths || !total_tokens || !total_positions || !n_cut || out_cap < 0) return fail(TKZ_E_ARG, kMsgBktPointers);
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(unit_offsets, n_docs, units != nullptr, kUnitDocs, &total));
    *total_tokens = 0; *total_positions = 0; *n_cut = 0;
    const PadCall pc{bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, nullptr, nullptr, nullptr, nullptr, nullptr};
    const BktCall bc{bucket_rows, order, nullptr, nullptr, nullptr, nullptr};
    Lease lease(e);
    Workspace* ws = lease.ws;
    if (total == 0) {                                                   // (no units: the offsets, all 0, are byte offsets as they are -- the framing is still laid out)
        TKZ_TRY(check_empty_docs(unit_offsets, n_docs, kUnitDocs, nullptr));
        TKZ_TRY(stage_in(ws, nullptr, 0, unit_offsets, n_docs));
        return bucketed_staged(e, ws, staged_call(ws, n_docs, 0, 0), pc, bc, sp, out_ids, out_cap, mask, pos, lens, out_offsets, order_out, rank, bucket_offsets, bucket_widths,
                               total_tokens, total_positions, n_cut);
    }
    U16Stage& U = ws->u16[0];
    const bool with_repl = sp && sp->fffd;
    HIP_TRY(U.ensure(total, n_docs, &ws->bytes_allocated, with_repl));
    HIP_TRY(hipMemcpy(U.units.p, units, (size_t)total * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U.offs.p, unit_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    const tkz::Launch L{nullptr, nullptr, ws};
    HIP_TRY(u16_measure(U, L, total, n_docs));
    HIP_TRY(hipStreamSynchronize(nullptr));
    int64_t nbytes = 0;                                                 // the batch as UTF-8
    TKZ_TRY(u16_write(U, L, total, n_docs, with_repl, &ws->bytes_allocated, &nbytes));
    BatchCall c{U.bytes.as<uint8_t>(), U.boffs.as<int64_t>(), n_docs, nbytes, nullptr, 0, nullptr, nullptr};
    if (with_repl) c.d_repl = U.repl.as<uint64_t>();
    return bucketed_staged(e, ws, c, pc, bc, sp, out_ids, out_cap, mask, pos, lens, out_offsets, order_out, rank, bucket_offsets, bucket_widths, total_tokens, total_positions,
                           n_cut);
}
void tkz_encoder_bucketed_calls(const tkz_encoder* e, int64_t* calls) {
    if (calls) *calls = e ? e->bucketed_calls.load() : 0;
}

// ---- token-budget buckets: the padded rows of the documents sorted by length, cut into buckets of at most token_budget positions and bucket_rows rows (tkz.h: the rule) ----

namespace {
tkz_status check_tbk_args(int64_t max_len, int64_t token_budget, int64_t bucket_cap, int64_t n_docs) {
    if (token_budget < max_len || token_budget > ((int64_t)1 << 62)) return fail(TKZ_E_ARG, "budgeted rows: token_budget must be in [max_len, 2^62]");
    if (bucket_cap < 0) return fail(TKZ_E_ARG, "budgeted rows: negative bucket_cap");
    if (n_docs > (int64_t)INT32_MAX) return fail(TKZ_E_ARG, "budgeted rows: more than 2^31 - 1 documents");      // (the buckets of a run are counted in 32 bits)
    return TKZ_OK;
}
const char* const kMsgTbkPointers = "budgeted rows: null ids, lens, order, bucket table or scalar pointer";
// the budgeted call on device buffers, on a workspace the entry holds: the bucketed call's sequence up to the sort, then the runs, the chain, the table and the rows
tkz_status budgeted_on_device(tkz_encoder* e, Workspace* ws, BatchCall c, PadCall pc, BktCall bc, TbkCall tc, const SpecialCall* sp, int64_t* total_tokens,
                              int64_t* total_positions, int64_t* n_cut, int64_t* n_buckets) {
    int64_t* acc = &ws->bytes_allocated;
    if (c.n_docs < 0 || c.total < 0 || c.out_cap < 0) return fail(TKZ_E_ARG, "negative size");
    const int64_t n = std::max<int64_t>(c.n_docs, 1), nt = tkz::bkt_sort_tiles(c.n_docs), nb = tc.table_cap(c.n_docs);
    const int64_t rc = tkz::tbk_run_cap(c.n_docs, pc.max_len, pc.pad_multiple), ng = tkz::tbk_mark_groups(c.n_docs);
    if (c.total > 0) HIP_TRY(ws->pd_ids.ensure((size_t)c.total * 4, acc));
    HIP_TRY(ws->pd_offs.ensure((size_t)(c.n_docs + 1) * 8, acc));
    HIP_TRY(ws->pd_src.ensure((size_t)n * 8, acc));
    HIP_TRY(ws->pd_part.ensure((size_t)tkz::kPadGridMax * 12, acc));
    HIP_TRY(ws->bk_keys.ensure((size_t)n * 3 * 4, acc));      // (key_a, key_b, slen)
    HIP_TRY(ws->bk_idx.ensure((size_t)n * 3 * 8, acc));       // (idx_a, idx_b, ssrc)
    HIP_TRY(ws->bk_hist.ensure((size_t)nt * 256 * 4, acc));
    HIP_TRY(ws->bk_base.ensure((size_t)(nt * 256 + 1) * 8, acc));
    HIP_TRY(ws->bk_bsum.ensure((size_t)(std::max(std::max(nt * 256, nb), std::max(rc, ng)) / tkz::kScanBlock + 2) * 8, acc));
    HIP_TRY(ws->bk_cnt.ensure((size_t)std::max<int64_t>(nb, 1) * 8, acc));
    HIP_TRY(ws->bk_boffs.ensure((size_t)(nb + 1) * 8, acc));
    HIP_TRY(ws->tb_marks.ensure((size_t)ng * 12, acc));
    HIP_TRY(ws->tb_runs.ensure((size_t)rc * 56, acc));
    HIP_TRY(ws->tb_rows.ensure((size_t)(nb + 1) * 8 + (size_t)std::max<int64_t>(nb, 1) * 4, acc));
    HIP_TRY(ws->tb_fig.ensure(32, acc));
    int64_t p = 0, cut = 0, buckets = 0;
    pc.width = &p; pc.n_cut = &cut; tc.n_buckets = &buckets;
    c.kind = CallKind::Budgeted; c.padded = &pc; c.bucketed = &bc; c.budgeted = &tc; c.special = sp;
    const tkz_status st = encode_device(e, ws, c, kCallWhole, total_tokens);
    if (total_positions) *total_positions = p;
    if (n_cut) *n_cut = cut;
    if (n_buckets) *n_buckets = buckets;
    if (st == TKZ_OK) { ++e->budgeted_calls; if (sp) ++e->spec_batches; }
    return st;
}
// The second half of a budgeted host entry, with the batch on the device as UTF-8: staging as bucketed_staged, and for the three bucket arrays at
// min(n_docs, bucket_cap) buckets; ONE budgeted call, the results back -- P entries of the rows, n_buckets of the bucket arrays, never the uncut ids.
tkz_status budgeted_staged(tkz_encoder* e, Workspace* ws, BatchCall c, PadCall pc, BktCall bc, TbkCall tc, const SpecialCall* sp, int32_t* out_ids, int64_t out_cap,
                           uint8_t* mask, int32_t* pos, int32_t* lens, int64_t* out_offsets, int64_t* order, int64_t* rank, int64_t* bucket_offsets, int64_t* bucket_rows_out,
                           int32_t* bucket_widths, int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut, int64_t* n_buckets) {
    const int64_t n_docs = c.n_docs, nb = tc.table_cap(n_docs);
    const bool fits = n_docs == 0 || out_cap / pc.max_len >= n_docs;      // (n_docs * max_len always suffices: more capacity is never used)
    c.out_cap = fits ? n_docs * pc.max_len : out_cap;
    tc.bucket_cap = nb;                                                  // (n_docs buckets always suffice likewise)
    const int64_t cap = std::max<int64_t>(c.out_cap, 1), nl = std::max<int64_t>(n_docs, 1);
    TKZ_TRY(stage_out(ws, n_docs, c.out_cap, out_offsets != nullptr));
    HIP_TRY(ws->pd_stage.ensure((size_t)(pos ? cap : 0) * 4 + (size_t)nl * 4 + (size_t)(mask ? cap : 0), &ws->bytes_allocated));
    HIP_TRY(ws->tb_stage.ensure((size_t)nl * 16 + (size_t)(nb + 1) * 20, &ws->bytes_allocated));
    int32_t* const d_pos = ws->pd_stage.as<int32_t>();
    int32_t* const d_lens = d_pos + (pos ? cap : 0);
    uint8_t* const d_mask = reinterpret_cast<uint8_t*>(d_lens + nl);
    int64_t* const d_order = ws->tb_stage.as<int64_t>();
    int64_t* const d_rank = d_order + nl;
    int64_t* const d_boffs = d_rank + nl;
    int64_t* const d_brows = d_boffs + nb + 1;
    int32_t* const d_widths = reinterpret_cast<int32_t*>(d_brows + nb + 1);
    c.d_out = ws->s_out[0].as<int32_t>(); c.d_out_offs = out_offsets ? ws->s_outoffs[0].as<int64_t>() : nullptr;
    pc.d_mask = mask ? d_mask : nullptr; pc.d_pos = pos ? d_pos : nullptr; pc.d_lens = d_lens;
    bc.d_order = d_order; bc.d_rank = rank ? d_rank : nullptr; bc.d_bucket_offs = d_boffs; bc.d_bucket_widths = d_widths; tc.d_bucket_rows = d_brows;
    const tkz_status st = budgeted_on_device(e, ws, c, pc, bc, tc, sp, total_tokens, total_positions, n_cut, n_buckets);
    if (st != TKZ_OK) return st;
    const int64_t n = *total_positions, k = *n_buckets;
    TKZ_TRY(fetch(ws, out_ids, n, out_offsets, n_docs));
    HIP_TRY(hipMemcpy(bucket_offsets, d_boffs, (size_t)(k + 1) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(bucket_rows_out, d_brows, (size_t)(k + 1) * 8, hipMemcpyDeviceToHost));
    if (n_docs) {
        HIP_TRY(hipMemcpy(lens, d_lens, (size_t)n_docs * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(order, d_order, (size_t)n_docs * 8, hipMemcpyDeviceToHost));
        if (rank) HIP_TRY(hipMemcpy(rank, d_rank, (size_t)n_docs * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(bucket_widths, d_widths, (size_t)k * 4, hipMemcpyDeviceToHost));
    }
    if (pos && n) HIP_TRY(hipMemcpy(pos, d_pos, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (mask && n) HIP_TRY(hipMemcpy(mask, d_mask, (size_t)n, hipMemcpyDeviceToHost));
    return TKZ_OK;
}
}  // namespace

tkz_status tkz_encode_batch_budgeted_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                            const int32_t* allowed, int32_t n_allowed, int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side,
                                            int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int64_t token_budget, int64_t bucket_rows, int32_t order,
                                            int32_t* d_out_ids, int64_t out_cap, uint8_t* d_mask, int32_t* d_pos, int32_t* d_lens, int64_t* d_out_offsets,
                                            int64_t* d_order, int64_t* d_rank, int64_t* d_bucket_offsets, int64_t* d_bucket_rows, int32_t* d_bucket_widths,
                                            int64_t bucket_cap, void* hip_stream, int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut, int64_t* n_buckets) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pad_args(bos_id, eos_id, max_len, cut_side, pad_side, pad_multiple));
    TKZ_TRY(check_bkt_args(bucket_rows, order));
    TKZ_TRY(check_tbk_args(max_len, token_budget, bucket_cap, n_docs));
    if (!d_out_ids || !d_lens || !d_order || !d_bucket_offsets || !d_bucket_rows || !d_bucket_widths || !total_tokens || !total_positions || !n_cut || !n_buckets)
        return fail(TKZ_E_ARG, kMsgTbkPointers);
    *total_tokens = 0; *total_positions = 0; *n_cut = 0; *n_buckets = 0;
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    if (!d_doc_offsets || (total_bytes > 0 && !d_bytes)) return fail(TKZ_E_ARG, "null device buffer");      // (d_out_offsets may be null here)
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(TKZ_E_ARG, "d_bytes must be 16-byte aligned");
    Lease lease(e);
    return budgeted_on_device(e, lease.ws, c, PadCall{bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, d_mask, d_pos, d_lens, nullptr, nullptr},
                              BktCall{bucket_rows, order, d_order, d_rank, d_bucket_offsets, d_bucket_widths}, TbkCall{token_budget, bucket_cap, d_bucket_rows, nullptr}, sp,
                              total_tokens, total_positions, n_cut, n_buckets);
}

tkz_status tkz_encode_batch_budgeted_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                          int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                          int64_t token_budget, int64_t bucket_rows, int32_t order, int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos,
                                          int32_t* lens, int64_t* out_offsets, int64_t* order_out, int64_t* rank, int64_t* bucket_offsets, int64_t* bucket_rows_out,
                                          int32_t* bucket_widths, int64_t bucket_cap, int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut, int64_t* n_buckets) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pad_args(bos_id, eos_id, max_len, cut_side, pad_side, pad_multiple));
    TKZ_TRY(check_bkt_args(bucket_rows, order));
    TKZ_TRY(check_tbk_args(max_len, token_budget, bucket_cap, n_docs));
    if (!out_ids || !lens || !order_out || !bucket_offsets || !bucket_rows_out || !bucket_widths || !total_tokens || !total_positions || !n_cut || !n_buckets || out_cap < 0)
        return fail(TKZ_E_ARG, kMsgTbkPointers);
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(doc_offsets, n_docs, bytes != nullptr, kSizedDocs, &total));
    if (total == 0) TKZ_TRY(check_empty_docs(doc_offsets, n_docs, kSizedDocs, nullptr));      // (... and the device call runs all the same)
    *total_tokens = 0; *total_positions = 0; *n_cut = 0; *n_buckets = 0;
    // the whole batch is staged and the result copied from ONE call of the device entry, as tkz_encode_batch_bucketed_utf8 does
    Lease lease(e);
    Workspace* ws = lease.ws;
    TKZ_TRY(stage_in(ws, bytes, total, doc_offsets, n_docs));
    return budgeted_staged(e, ws, staged_call(ws, n_docs, total, 0), PadCall{bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, nullptr, nullptr, nullptr, nullptr, nullptr},
                           BktCall{bucket_rows, order, nullptr, nullptr, nullptr, nullptr}, TbkCall{token_budget, bucket_cap, nullptr, nullptr}, sp, out_ids, out_cap, mask, pos,
                           lens, out_offsets, order_out, rank, bucket_offsets, bucket_rows_out, bucket_widths, total_tokens, total_positions, n_cut, n_buckets);
}

// The same for UTF-16 documents: code units staged and transcoded on the device as tkz_encode_batch_bucketed_utf16 does.
tkz_status tkz_encode_batch_budgeted_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                           int32_t bos_id, int32_t eos_id, int64_t max_len, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple,
                                           int64_t token_budget, int64_t bucket_rows, int32_t order, int32_t* out_ids, int64_t out_cap, uint8_t* mask, int32_t* pos,
                                           int32_t* lens, int64_t* out_offsets, int64_t* order_out, int64_t* rank, int64_t* bucket_offsets, int64_t* bucket_rows_out,
                                           int32_t* bucket_widths, int64_t bucket_cap, int64_t* total_tokens, int64_t* total_positions, int64_t* n_cut, int64_t* n_buckets) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pad_args(bos_id, eos_id, max_len, cut_side, pad_side, pad_multiple));
    TKZ_TRY(check_bkt_args(bucket_rows, order));
    TKZ_TRY(check_tbk_args(max_len, token_budget, bucket_cap, n_docs));
    if (!out_ids || !lens || !order_out || !bucket_offsets || !bucket_rows_out || !bucket_widths || !total_tokens || !total_positions || !n_cut || !n_buckets || out_cap < 0)
        return fail(TKZ_E_ARG, kMsgTbkPointers);
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(unit_offsets, n_docs, units != nullptr, kUnitDocs, &total));
    *total_tokens = 0; *total_positions = 0; *n_cut = 0; *n_buckets = 0;
    const PadCall pc{bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, nullptr, nullptr, nullptr, nullptr, nullptr};
    const BktCall bc{bucket_rows, order, nullptr, nullptr, nullptr, nullptr};
    const TbkCall tc{token_budget, bucket_cap, nullptr, nullptr};
    Lease lease(e);
    Workspace* ws = lease.ws;
    if (total == 0) {                                                   // (no units: the offsets, all 0, are byte offsets as they are -- the framing is still laid out)
        TKZ_TRY(check_empty_docs(unit_offsets, n_docs, kUnitDocs, nullptr));
        TKZ_TRY(stage_in(ws, nullptr, 0, unit_offsets, n_docs));
        return budgeted_staged(e, ws, staged_call(ws, n_docs, 0, 0), pc, bc, tc, sp, out_ids, out_cap, mask, pos, lens, out_offsets, order_out, rank, bucket_offsets,
                               bucket_rows_out, bucket_widths, total_tokens, total_positions, n_cut, n_buckets);
    }
    U16Stage& U = ws->u16[0];
    const bool with_repl = sp && sp->fffd;
    HIP_TRY(U.ensure(total, n_docs, &ws->bytes_allocated, with_repl));
    HIP_TRY(hipMemcpy(U.units.p, units, (size_t)total * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U.offs.p, unit_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    const tkz::Launch L{nullptr, nullptr, ws};
    HIP_TRY(u16_measure(U, L, total, n_docs));
    HIP_TRY(hipStreamSynchronize(nullptr));
    int64_t nbytes = 0;                                                 // the batch as UTF-8
    TKZ_TRY(u16_write(U, L, total, n_docs, with_repl, &ws->bytes_allocated, &nbytes));
    BatchCall c{U.bytes.as<uint8_t>(), U.boffs.as<int64_t>(), n_docs, nbytes, nullptr, 0, nullptr, nullptr};
    if (with_repl) c.d_repl = U.repl.as<uint64_t>();
    return budgeted_staged(e, ws, c, pc, bc, tc, sp, out_ids, out_cap, mask, pos, lens, out_offsets, order_out, rank, bucket_offsets, bucket_rows_out, bucket_widths,
                           total_tokens, total_positions, n_cut, n_buckets);
}
void tkz_encoder_budgeted_calls(const tkz_encoder* e, int64_t* calls) {
    if (calls) *calls = e ? e->budgeted_calls.load() : 0;
}

// ---- pair rows: documents 2p and 2p + 1 as the two texts of row p -- cut to max_len by a strategy, [bos] A sep x s B [eos], padded to the common width (tkz.h: the rule) ----

namespace {
tkz_status check_pair_args(int64_t n_docs, int32_t bos_id, int32_t sep_id, int32_t sep_count, int32_t eos_id, int64_t max_len, int32_t strategy, int32_t cut_side,
                           int32_t pad_side, int64_t pad_multiple) {
    if (n_docs >= 0 && (n_docs & 1)) return fail(TKZ_E_ARG, "pair rows: n_docs must be even -- documents 2p and 2p + 1 are the two texts of pair p");
    if (bos_id < -1 || eos_id < -1) return fail(TKZ_E_ARG, "pair rows: bos_id and eos_id are -1 (none) or an id >= 0");
    if (sep_count < 0 || sep_count > 2) return fail(TKZ_E_ARG, "pair rows: sep_count must be 0, 1 or 2");
    if (sep_count > 0 && sep_id < 0) return fail(TKZ_E_ARG, "pair rows: sep_id must be an id >= 0 when sep_count > 0");
    const int64_t f = (bos_id >= 0) + (eos_id >= 0) + sep_count;
    if (max_len < std::max<int64_t>(1, f) || max_len > (int64_t)INT32_MAX) return fail(TKZ_E_ARG, "pair rows: max_len must be in [max(1, framing ids), 2^31 - 1]");
    if (strategy != TKZ_PAIR_LONGEST_FIRST && strategy != TKZ_PAIR_ONLY_FIRST && strategy != TKZ_PAIR_ONLY_SECOND)
        return fail(TKZ_E_ARG, "pair rows: strategy must be TKZ_PAIR_LONGEST_FIRST, TKZ_PAIR_ONLY_FIRST or TKZ_PAIR_ONLY_SECOND");
    if (cut_side != TKZ_TRIM_SUFFIX && cut_side != TKZ_TRIM_PREFIX) return fail(TKZ_E_ARG, "pair rows: cut_side must be TKZ_TRIM_SUFFIX or TKZ_TRIM_PREFIX");
    if (pad_side != TKZ_PAD_RIGHT && pad_side != TKZ_PAD_LEFT) return fail(TKZ_E_ARG, "pair rows: pad_side must be TKZ_PAD_RIGHT or TKZ_PAD_LEFT");
    if (pad_multiple < 0 || pad_multiple > (int64_t)INT32_MAX) return fail(TKZ_E_ARG, "pair rows: pad_multiple must be in [0, 2^31 - 1]");
    return TKZ_OK;
}
const char* const kMsgPairPointers = "pair rows: null ids, lens or scalar pointer";
// the pair call on device buffers, on a workspace the entry holds: the plain launch sequence with the uncut ids and offsets in the workspace, then the rows
// (enqueue_attempt)
tkz_status pairs_on_device(tkz_encoder* e, Workspace* ws, BatchCall c, PairCall pc, const SpecialCall* sp, int64_t* total_tokens, int64_t* width, int64_t* n_cut) {
    int64_t* acc = &ws->bytes_allocated;
    if (c.n_docs < 0 || c.total < 0 || c.out_cap < 0) return fail(TKZ_E_ARG, "negative size");
    const int64_t np = std::max<int64_t>(c.n_docs / 2, 1);
    if (c.total > 0) HIP_TRY(ws->pr_ids.ensure((size_t)c.total * 4, acc));
    HIP_TRY(ws->pr_offs.ensure((size_t)(c.n_docs + 1) * 8, acc));
    HIP_TRY(ws->pr_src.ensure((size_t)np * 24, acc));
    HIP_TRY(ws->pr_part.ensure((size_t)tkz::kPairGridMax * 12, acc));
    int64_t w = 0, cut = 0;
    pc.width = &w; pc.n_cut = &cut;
    c.kind = CallKind::Pairs; c.pairs = &pc; c.special = sp;
    const tkz_status st = encode_device(e, ws, c, kCallWhole, total_tokens);
    if (width) *width = w;
    if (n_cut) *n_cut = cut;
    if (st == TKZ_OK) { ++e->pairs_calls; if (sp) ++e->spec_batches; }
    return st;
}
// The second half of a pair host entry, with the batch on the device as UTF-8 (c: its bytes and byte offsets): staging for the rows, the offsets, pos, lens, kept,
// the mask and the types, ONE pair call, the results back -- n_pairs * W entries of each, never the uncut ids.
tkz_status pairs_staged(tkz_encoder* e, Workspace* ws, BatchCall c, PairCall pc, const SpecialCall* sp, int32_t* out_ids, int64_t out_cap, uint8_t* mask, uint8_t* type_ids,
                        int32_t* pos, int32_t* lens, int32_t* kept, int64_t* out_offsets, int64_t* total_tokens, int64_t* width, int64_t* n_cut) {
    const int64_t n_docs = c.n_docs, n_pairs = n_docs / 2;
    const bool fits = n_pairs == 0 || out_cap / pc.max_len >= n_pairs;      // (n_pairs * max_len always suffices: more capacity is never used)
    c.out_cap = fits ? n_pairs * pc.max_len : out_cap;
    const int64_t cap = std::max<int64_t>(c.out_cap, 1), nl = std::max<int64_t>(n_pairs, 1);
    TKZ_TRY(stage_out(ws, n_docs, c.out_cap, out_offsets != nullptr));
    HIP_TRY(ws->pr_stage.ensure((size_t)(pos ? cap : 0) * 4 + (size_t)nl * 4 + (size_t)(kept ? 2 * nl : 0) * 4 + (size_t)(mask ? cap : 0) + (size_t)(type_ids ? cap : 0),
                                &ws->bytes_allocated));
    int32_t* const d_pos = ws->pr_stage.as<int32_t>();
    int32_t* const d_lens = d_pos + (pos ? cap : 0);
    int32_t* const d_kept = d_lens + nl;
    uint8_t* const d_mask = reinterpret_cast<uint8_t*>(d_kept + (kept ? 2 * nl : 0));
    uint8_t* const d_types = d_mask + (mask ? cap : 0);
    c.d_out = ws->s_out[0].as<int32_t>(); c.d_out_offs = out_offsets ? ws->s_outoffs[0].as<int64_t>() : nullptr;
    pc.d_mask = mask ? d_mask : nullptr; pc.d_types = type_ids ? d_types : nullptr; pc.d_pos = pos ? d_pos : nullptr; pc.d_lens = d_lens; pc.d_kept = kept ? d_kept : nullptr;
    const tkz_status st = pairs_on_device(e, ws, c, pc, sp, total_tokens, width, n_cut);
    if (st != TKZ_OK) return st;
    const int64_t n = n_pairs * *width;
    TKZ_TRY(fetch(ws, out_ids, n, out_offsets, n_docs));
    if (n_pairs) HIP_TRY(hipMemcpy(lens, d_lens, (size_t)n_pairs * 4, hipMemcpyDeviceToHost));
    if (kept && n_docs) HIP_TRY(hipMemcpy(kept, d_kept, (size_t)n_docs * 4, hipMemcpyDeviceToHost));
    if (pos && n) HIP_TRY(hipMemcpy(pos, d_pos, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (mask && n) HIP_TRY(hipMemcpy(mask, d_mask, (size_t)n, hipMemcpyDeviceToHost));
    if (type_ids && n) HIP_TRY(hipMemcpy(type_ids, d_types, (size_t)n, hipMemcpyDeviceToHost));
    return TKZ_OK;
}
}  // namespace

tkz_status tkz_encode_batch_pairs_device(tkz_encoder* e, const uint8_t* d_bytes, const int64_t* d_doc_offsets, int64_t n_docs, int64_t total_bytes,
                                         const int32_t* allowed, int32_t n_allowed, int32_t bos_id, int32_t sep_id, int32_t sep_count, int32_t eos_id, int64_t max_len,
                                         int32_t strategy, int32_t cut_side, int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int32_t* d_out_ids, int64_t out_cap,
                                         uint8_t* d_mask, uint8_t* d_type_ids, int32_t* d_pos, int32_t* d_lens, int32_t* d_kept, int64_t* d_out_offsets, void* hip_stream,
                                         int64_t* total_tokens, int64_t* width, int64_t* n_cut) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pair_args(n_docs, bos_id, sep_id, sep_count, eos_id, max_len, strategy, cut_side, pad_side, pad_multiple));
    if (!d_out_ids || !d_lens || !total_tokens || !width || !n_cut) return fail(TKZ_E_ARG, kMsgPairPointers);
    *total_tokens = 0; *width = 0; *n_cut = 0;
    BatchCall c{d_bytes, d_doc_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream)};
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    if (!d_doc_offsets || (total_bytes > 0 && !d_bytes)) return fail(TKZ_E_ARG, "null device buffer");      // (d_out_offsets may be null here)
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(TKZ_E_ARG, "d_bytes must be 16-byte aligned");
    Lease lease(e);
    return pairs_on_device(e, lease.ws, c, PairCall{bos_id, sep_id, sep_count, eos_id, max_len, strategy, cut_side, pad_side, pad_id, pad_multiple, d_mask, d_type_ids, d_pos,
                                                    d_lens, d_kept, nullptr, nullptr}, sp, total_tokens, width, n_cut);
}

tkz_status tkz_encode_batch_pairs_utf8(tkz_encoder* e, const uint8_t* bytes, const int64_t* doc_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                       int32_t bos_id, int32_t sep_id, int32_t sep_count, int32_t eos_id, int64_t max_len, int32_t strategy, int32_t cut_side,
                                       int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int32_t* out_ids, int64_t out_cap, uint8_t* mask, uint8_t* type_ids,
                                       int32_t* pos, int32_t* lens, int32_t* kept, int64_t* out_offsets, int64_t* total_tokens, int64_t* width, int64_t* n_cut) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pair_args(n_docs, bos_id, sep_id, sep_count, eos_id, max_len, strategy, cut_side, pad_side, pad_multiple));
    if (!out_ids || !lens || !total_tokens || !width || !n_cut || out_cap < 0) return fail(TKZ_E_ARG, kMsgPairPointers);
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(doc_offsets, n_docs, bytes != nullptr, kSizedDocs, &total));
    if (total == 0) TKZ_TRY(check_empty_docs(doc_offsets, n_docs, kSizedDocs, nullptr));      // (... and the device call runs all the same)
    *total_tokens = 0; *width = 0; *n_cut = 0;
    // the whole batch is staged and the result copied from ONE call of the device entry, as tkz_encode_batch_padded_utf8 does
    Lease lease(e);
    Workspace* ws = lease.ws;
    TKZ_TRY(stage_in(ws, bytes, total, doc_offsets, n_docs));
    return pairs_staged(e, ws, staged_call(ws, n_docs, total, 0),
                        PairCall{bos_id, sep_id, sep_count, eos_id, max_len, strategy, cut_side, pad_side, pad_id, pad_multiple, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr}, sp, out_ids, out_cap, mask, type_ids, pos, lens, kept, out_offsets, total_tokens, width, n_cut);
}

// The same for UTF-16 documents: code units staged and transcoded on the device as tkz_encode_batch_padded_utf16 does.
tkz_status tkz_encode_batch_pairs_utf16(tkz_encoder* e, const uint16_t* units, const int64_t* unit_offsets, int64_t n_docs, const int32_t* allowed, int32_t n_allowed,
                                        int32_t bos_id, int32_t sep_id, int32_t sep_count, int32_t eos_id, int64_t max_len, int32_t strategy, int32_t cut_side,
                                        int32_t pad_side, int32_t pad_id, int64_t pad_multiple, int32_t* out_ids, int64_t out_cap, uint8_t* mask, uint8_t* type_ids,
                                        int32_t* pos, int32_t* lens, int32_t* kept, int64_t* out_offsets, int64_t* total_tokens, int64_t* width, int64_t* n_cut) {
    SpecialCall sc; const SpecialCall* sp;
    TKZ_TRY(special_call(e, allowed, n_allowed, &sc, &sp));
    TKZ_TRY(check_pair_args(n_docs, bos_id, sep_id, sep_count, eos_id, max_len, strategy, cut_side, pad_side, pad_multiple));
    if (!out_ids || !lens || !total_tokens || !width || !n_cut || out_cap < 0) return fail(TKZ_E_ARG, kMsgPairPointers);
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    int64_t total = 0;
    TKZ_TRY(check_host_docs(unit_offsets, n_docs, units != nullptr, kUnitDocs, &total));
    *total_tokens = 0; *width = 0; *n_cut = 0;
    const PairCall pc{bos_id, sep_id, sep_count, eos_id, max_len, strategy, cut_side, pad_side, pad_id, pad_multiple, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    Lease lease(e);
    Workspace* ws = lease.ws;
    if (total == 0) {                                                   // (no units: the offsets, all 0, are byte offsets as they are -- the framing is still laid out)
        TKZ_TRY(check_empty_docs(unit_offsets, n_docs, kUnitDocs, nullptr));
        TKZ_TRY(stage_in(ws, nullptr, 0, unit_offsets, n_docs));
        return pairs_staged(e, ws, staged_call(ws, n_docs, 0, 0), pc, sp, out_ids, out_cap, mask, type_ids, pos, lens, kept, out_offsets, total_tokens, width, n_cut);
    }
    U16Stage& U = ws->u16[0];
    const bool with_repl = sp && sp->fffd;
    HIP_TRY(U.ensure(total, n_docs, &ws->bytes_allocated, with_repl));
    HIP_TRY(hipMemcpy(U.units.p, units, (size_t)total * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U.offs.p, unit_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    const tkz::Launch L{nullptr, nullptr, ws};
    HIP_TRY(u16_measure(U, L, total, n_docs));
    HIP_TRY(hipStreamSynchronize(nullptr));
    int64_t nbytes = 0;                                                 // the batch as UTF-8
    TKZ_TRY(u16_write(U, L, total, n_docs, with_repl, &ws->bytes_allocated, &nbytes));
    BatchCall c{U.bytes.as<uint8_t>(), U.boffs.as<int64_t>(), n_docs, nbytes, nullptr, 0, nullptr, nullptr};
    if (with_repl) c.d_repl = U.repl.as<uint64_t>();
    return pairs_staged(e, ws, c, pc, sp, out_ids, out_cap, mask, type_ids, pos, lens, kept, out_offsets, total_tokens, width, n_cut);
}
void tkz_encoder_pairs_calls(const tkz_encoder* e, int64_t* calls) {
    if (calls) *calls = e ? e->pairs_calls.load() : 0;
}

// ---- Decode (TikTokenizer.cs:586-604) ----------------------------------------------------------------

tkz_status tkz_encoder_set_special_tokens(tkz_encoder* e, const int32_t* ids, const uint8_t* literals_utf8, const int64_t* literal_offsets, int32_t n) {
    DeviceScope scope;
    tkz_status st = check_encoder(e, scope);
    if (st != TKZ_OK) return st;
    if (n < 0 || (n > 0 && (!ids || !literal_offsets || (!literals_utf8 && literal_offsets[n] > 0)))) return fail(TKZ_E_ARG, "bad special-token arguments");
    std::lock_guard<std::mutex> lock(e->mu);
    std::vector<std::pair<int32_t, std::string>> sp;
    for (int32_t i = 0; i < n; ++i) {
        if (literal_offsets[i + 1] < literal_offsets[i] || literal_offsets[i] < 0) return fail(TKZ_E_ARG, "literal offsets must be non-decreasing");
        sp.emplace_back(ids[i], std::string(reinterpret_cast<const char*>(literals_utf8) + literal_offsets[i], (size_t)(literal_offsets[i + 1] - literal_offsets[i])));
    }
    e->dec_special.swap(sp);
    st = build_decode_table(e);
    return st != TKZ_OK ? st : build_literal_table(e);
}

namespace {
// The head of both decoders, on `stream`: the checks of the sizes, the length scan's buffers, the byte length of every id and their scan.  What it leaves:
// d_grp / d_tbase (the per-group and per-tile bases dec_write places by) and, in the counter block d_counters (a LenCounters), the byte total.
tkz_status decode_lengths(tkz_encoder* e, Workspace* ws, const int32_t* d_ids, int64_t n_docs, int64_t total_ids, int64_t out_cap, hipStream_t stream) {
    using namespace tkz;
    if (n_docs < 0 || total_ids < 0 || out_cap < 0) return fail(TKZ_E_ARG, "negative size");
    if (n_docs == 0 && total_ids != 0) return fail(TKZ_E_ARG, "ids without documents");
    int64_t* acc = &ws->bytes_allocated;
    const int64_t ntiles = std::max<int64_t>(1, dec_tiles(total_ids)), nblk = (ntiles + kScanBlock - 1) / kScanBlock;
    HIP_TRY(ws->d_grp.ensure((size_t)ntiles * 64 * 4, acc));
    HIP_TRY(ws->d_tsum.ensure((size_t)ntiles * 4, acc));
    HIP_TRY(ws->d_tbase.ensure((size_t)ntiles * 8, acc));
    HIP_TRY(ws->d_bsum.ensure((size_t)(nblk + 1) * 8, acc));
    HIP_TRY(ws->d_counters.ensure(64, acc));
    if (!ws->h_counters) HIP_TRY(hipHostMalloc((void**)&ws->h_counters, sizeof(CounterBlock), 0));
    const Launch L{stream, nullptr, ws};
    HIP_TRY(hipMemsetAsync(ws->d_counters.p, 0, 64, stream));
    launch_dec_len(L, e->D, d_ids, total_ids, ntiles, ws->d_grp.as<int32_t>(), ws->d_tsum.as<int32_t>());
    launch_scan(L, ws->d_tsum.as<int32_t>(), ntiles, ws->d_bsum.as<int64_t>(), ws->d_tbase.as<int64_t>(), &ws->d_counters.as<LenCounters>()->grand, -1);
    return TKZ_OK;
}
// the first n bytes of that block on the host, once the stream has drained
tkz_status fetch_len_counters(Workspace* ws, hipStream_t stream, size_t n, LenCounters* h) {
    HIP_TRY(hipMemcpyAsync(ws->h_counters, ws->d_counters.p, n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipGetLastError());
    memcpy(h, ws->h_counters, n);
    return TKZ_OK;
}

// lengths -> scan -> bytes + document offsets, all on `stream` with ONE wait at the end; d_out may be null when only the size is wanted
tkz_status decode_device(tkz_encoder* e, Workspace* ws, const int32_t* d_ids, const int64_t* d_id_offs, int64_t n_docs, int64_t total_ids, uint8_t* d_out, int64_t out_cap,
                         int64_t* d_out_offs, hipStream_t stream, int64_t* total_bytes) {
    using namespace tkz;
    if (total_bytes) *total_bytes = 0;
    TKZ_TRY(decode_lengths(e, ws, d_ids, n_docs, total_ids, out_cap, stream));
    LenCounters* const blk = ws->d_counters.as<LenCounters>();
    launch_dec_write(Launch{stream, nullptr, ws}, e->D, d_ids, total_ids, std::max<int64_t>(1, dec_tiles(total_ids)), ws->d_tbase.as<int64_t>(), d_out, d_out ? out_cap : 0,
                     d_id_offs, n_docs, ws->d_grp.as<int32_t>(), &blk->grand, d_out_offs, &blk->err);
    LenCounters h{};
    TKZ_TRY(fetch_len_counters(ws, stream, 16, &h));
    if (h.err & kErrOffsets) return fail(TKZ_E_ARG, kMsgIdOffsets);
    if (total_bytes) *total_bytes = h.grand;
    if (h.grand > out_cap) return fail(TKZ_E_CAPACITY, "output capacity too small");
    return TKZ_OK;
}


// Decode + Encoding.UTF8.GetString: the byte decoder's lengths and scan, ONE wait for the byte total (the intermediate bytes are sized from it, not from
// total_ids x the longest key), the bytes and their offsets into the workspace, the document-start bitmap over them, then unit counts -> scan -> units + unit
// offsets.  own_units: null (d_out is the caller's), or the workspace buffer the host entry's units go to: sized here, to min(out_cap, bytes) -- a unit
// stands for at least one byte.
tkz_status decode_utf16_device(tkz_encoder* e, Workspace* ws, const int32_t* d_ids, const int64_t* d_id_offs, int64_t n_docs, int64_t total_ids, uint16_t* d_out,
                               int64_t out_cap, int64_t* d_out_offs, hipStream_t stream, int64_t* total_units, DevBuf* own_units = nullptr) {
    using namespace tkz;
    if (total_units) *total_units = 0;
    TKZ_TRY(decode_lengths(e, ws, d_ids, n_docs, total_ids, out_cap, stream));
    int64_t* acc = &ws->bytes_allocated;
    HIP_TRY(ws->d8_boffs.ensure((size_t)(n_docs + 1) * 8, acc));
    const Launch L{stream, nullptr, ws};
    LenCounters* const blk = ws->d_counters.as<LenCounters>();
    LenCounters h{};
    TKZ_TRY(fetch_len_counters(ws, stream, 16, &h));
    const int64_t nbytes = h.grand;                                     // the batch as (not necessarily well-formed) UTF-8
    const int64_t nw = nbytes / 64 + 1, nt8 = std::max<int64_t>(1, u8_tiles(nbytes)), nblk8 = (nt8 + kScanBlock - 1) / kScanBlock;
    HIP_TRY(ws->d8_bytes.ensure((size_t)nbytes + 64, acc));
    HIP_TRY(ws->d8_docbits.ensure((size_t)(nw + 8) * 8, acc));
    HIP_TRY(ws->d8_grp.ensure((size_t)nt8 * 64 * 4, acc));
    HIP_TRY(ws->d8_tsum.ensure((size_t)nt8 * 4, acc));
    HIP_TRY(ws->d8_tbase.ensure((size_t)nt8 * 8, acc));
    HIP_TRY(ws->d8_bsum.ensure((size_t)(nblk8 + 1) * 8, acc));
    if (own_units) {
        out_cap = std::min<int64_t>(out_cap, nbytes);
        HIP_TRY(own_units->ensure((size_t)std::max<int64_t>(out_cap, 1) * 2, acc));
        d_out = own_units->as<uint16_t>();
    }
    const uint8_t* bytes = ws->d8_bytes.as<uint8_t>();
    const uint64_t* docbits = ws->d8_docbits.as<uint64_t>();
    HIP_TRY(hipMemsetAsync(ws->d8_docbits.p, 0, (size_t)(nw + 8) * 8, stream));
    launch_dec_write(L, e->D, d_ids, total_ids, std::max<int64_t>(1, dec_tiles(total_ids)), ws->d_tbase.as<int64_t>(), ws->d8_bytes.as<uint8_t>(), nbytes, d_id_offs, n_docs,
                     ws->d_grp.as<int32_t>(), &blk->grand, ws->d8_boffs.as<int64_t>(), &blk->err);
    // (empty documents set no bit of their own; bad id offsets have set kErrOffsets above, and what is computed from their byte offsets is never used)
    launch_docmark(L, ws->d8_boffs.as<int64_t>(), n_docs, nbytes, ws->d8_docbits.as<uint64_t>(), &blk->err);
    launch_u8_len(L, bytes, nbytes, docbits, nw, nt8, ws->d8_grp.as<int32_t>(), ws->d8_tsum.as<int32_t>());
    launch_scan(L, ws->d8_tsum.as<int32_t>(), nt8, ws->d8_bsum.as<int64_t>(), ws->d8_tbase.as<int64_t>(), &blk->grand16, -1);
    launch_u8_write(L, bytes, nbytes, docbits, nw, nt8, ws->d8_tbase.as<int64_t>(), d_out, d_out ? out_cap : 0, ws->d8_boffs.as<int64_t>(), n_docs,
                    ws->d8_grp.as<int32_t>(), &blk->grand16, d_out_offs);
    TKZ_TRY(fetch_len_counters(ws, stream, sizeof h, &h));
    if (h.err & kErrOffsets) return fail(TKZ_E_ARG, kMsgIdOffsets);
    if (total_units) *total_units = h.grand16;
    if (h.grand16 > out_cap) return fail(TKZ_E_CAPACITY, "output capacity too small");
    return TKZ_OK;
}
// tkz_decode_batch and tkz_decode_batch_utf16 (utf16: `out` holds code units): ids and id offsets in, ONE call of the device decoder, items and offsets out
tkz_status decode_host(tkz_encoder* e, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs, void* out, int64_t out_cap, int64_t* out_offsets, int64_t* needed,
                       bool utf16) {
    DeviceScope scope;
    TKZ_TRY(check_encoder(e, scope));
    TKZ_TRY(check_host_outputs(out, out_cap, out_offsets, "null buffer"));
    int64_t total = 0, n_items = 0;
    TKZ_TRY(check_host_docs(id_offsets, n_docs, ids != nullptr, kIdDocs, &total));
    if (needed) *needed = 0;
    Lease lease(e);
    Workspace* ws = lease.ws;
    int64_t* acc = &ws->bytes_allocated;
    HIP_TRY(ws->d_ids.ensure((size_t)std::max<int64_t>(total, 1) * 4, acc));
    for (DevBuf* b : {&ws->d_idoffs, &ws->d_outoffs}) HIP_TRY(b->ensure((size_t)(n_docs + 1) * 8, acc));
    if (total) HIP_TRY(hipMemcpy(ws->d_ids.p, ids, (size_t)total * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ws->d_idoffs.p, id_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    DevBuf& items = utf16 ? ws->d8_units : ws->d_out;          // (the unit staging is sized inside decode_utf16_device, from the byte total)
    if (!utf16) {      // staging no larger than the result can be: an id yields at most the longest registered byte string, however large a hint out_cap is
        int64_t longest = 1;
        { std::lock_guard<std::mutex> lock(e->mu); for (const auto& kv : e->dec_special) longest = std::max<int64_t>(longest, (int64_t)kv.second.size()); }
        longest = std::max<int64_t>(longest, e->max_key_len);
        out_cap = std::min<int64_t>(out_cap, total * longest);
        HIP_TRY(items.ensure((size_t)std::max<int64_t>(out_cap, 1), acc));
    }
    const tkz_status st = utf16 ? decode_utf16_device(e, ws, ws->d_ids.as<int32_t>(), ws->d_idoffs.as<int64_t>(), n_docs, total, nullptr, out_cap, ws->d_outoffs.as<int64_t>(), nullptr, &n_items, &items)
                                : decode_device(e, ws, ws->d_ids.as<int32_t>(), ws->d_idoffs.as<int64_t>(), n_docs, total, items.as<uint8_t>(), out_cap, ws->d_outoffs.as<int64_t>(), nullptr, &n_items);
    if (needed) *needed = n_items;
    if (st != TKZ_OK) return st;
    if (n_items) HIP_TRY(hipMemcpy(out, items.p, (size_t)n_items * (utf16 ? 2 : 1), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_offsets, ws->d_outoffs.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost));
    return TKZ_OK;
}
tkz_status check_decode_device(tkz_encoder* e, DeviceScope& scope, const int32_t* d_ids, const int64_t* d_id_offsets, int64_t total_ids, const void* d_out, int64_t out_cap,
                               const int64_t* d_out_offsets) {
    TKZ_TRY(check_encoder(e, scope));
    if (!d_id_offsets || !d_out_offsets || (total_ids > 0 && !d_ids) || (out_cap > 0 && !d_out)) return fail(TKZ_E_ARG, "null device buffer");
    return TKZ_OK;
}
}  // namespace

tkz_status tkz_decode_batch_device(tkz_encoder* e, const int32_t* d_ids, const int64_t* d_id_offsets, int64_t n_docs, int64_t total_ids,
                                   uint8_t* d_out_bytes, int64_t out_cap, int64_t* d_out_offsets, void* hip_stream, int64_t* total_bytes) {
    DeviceScope scope;
    TKZ_TRY(check_decode_device(e, scope, d_ids, d_id_offsets, total_ids, d_out_bytes, out_cap, d_out_offsets));
    Lease lease(e);
    return decode_device(e, lease.ws, d_ids, d_id_offsets, n_docs, total_ids, d_out_bytes, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream), total_bytes);
}
tkz_status tkz_decode_batch_utf16_device(tkz_encoder* e, const int32_t* d_ids, const int64_t* d_id_offsets, int64_t n_docs, int64_t total_ids,
                                         uint16_t* d_out_units, int64_t out_cap, int64_t* d_out_offsets, void* hip_stream, int64_t* total_units) {
    DeviceScope scope;
    TKZ_TRY(check_decode_device(e, scope, d_ids, d_id_offsets, total_ids, d_out_units, out_cap, d_out_offsets));
    Lease lease(e);
    return decode_utf16_device(e, lease.ws, d_ids, d_id_offsets, n_docs, total_ids, d_out_units, out_cap, d_out_offsets, static_cast<hipStream_t>(hip_stream), total_units);
}

tkz_status tkz_decode_batch(tkz_encoder* e, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs, uint8_t* out_bytes, int64_t out_cap,
                            int64_t* out_offsets, int64_t* needed) {
    return decode_host(e, ids, id_offsets, n_docs, out_bytes, out_cap, out_offsets, needed, false);
}
tkz_status tkz_decode_batch_utf16(tkz_encoder* e, const int32_t* ids, const int64_t* id_offsets, int64_t n_docs, uint16_t* out_units, int64_t out_cap,
                                  int64_t* out_offsets, int64_t* needed) {
    return decode_host(e, ids, id_offsets, n_docs, out_units, out_cap, out_offsets, needed, true);
}

// ---- Decode of ONE id list in a single launch (k_dec_small) -----------------------------------------------------------------------------------
// ITokenizer.Decode(int[]) through the batch entries is two blocking uploads, a dozen launches, two waits and two blocking downloads whatever the size
// (decode_host + decode_utf16_device).  A list of at most kDecSmallRouteIds ids goes through ONE launch instead, as encode_small does it for a prompt: the ids
// are memcpy'd into a page-locked block, k_dec_small (one workgroup, all phases) reads them from there and writes the bytes or the code units and a result
// record back into it, one stream synchronisation, memcpy out.  The entry is validate (check_decode_one) -> the launch (decode_small) -> fetch
// (fetch_decode_small); a list the launch does not take, or hands back, is decode_host's with one document.
namespace {
constexpr size_t kDecSmallOffIds = 0, kDecSmallOffOut = (size_t)tkz::kDecSmallMaxIds * 4, kDecSmallOffRes = kDecSmallOffOut + (size_t)tkz::kDecSmallMaxBytes * 2,
                 kDecSmallBlock = kDecSmallOffRes + 256;
tkz_status check_decode_one(tkz_encoder* e, DeviceScope& scope, const int32_t* ids, int64_t n_ids, const void* out, int64_t out_cap, int64_t* n_out) {
    TKZ_TRY(check_encoder(e, scope));
    if (!n_out) return fail(TKZ_E_ARG, "null n_out");
    *n_out = 0;
    if (n_ids < 0 || out_cap < 0) return fail(TKZ_E_ARG, "negative size");
    if (n_ids > 0 && !ids) return fail(TKZ_E_ARG, "null ids");
    if (out_cap > 0 && !out) return fail(TKZ_E_ARG, "null buffer");
    return TKZ_OK;
}
// Returns TKZ_OK with *handled = false when the kernel hands the list back (it decodes to more than kDecSmallMaxBytes bytes): the caller takes the batch path.
tkz_status decode_small(tkz_encoder* e, Workspace* ws, const int32_t* ids, int64_t n_ids, bool utf16, int64_t* n_items, bool* handled) {
    using namespace tkz;
    *handled = false;
    int64_t* acc = &ws->bytes_allocated;
    if (utf16) {
        HIP_TRY(ws->ds_bytes.ensure((size_t)kDecSmallMaxBytes + 64, acc));
        HIP_TRY(ws->ds_docbits.ensure((size_t)(kDecSmallMaxBytes / 64 + 1 + 8) * 8, acc));
    }
    if (!ws->h_dsmall) HIP_TRY(hipHostMalloc((void**)&ws->h_dsmall, kDecSmallBlock, 0));
    if (!ws->st_small) HIP_TRY(hipStreamCreateWithFlags(&ws->st_small, hipStreamNonBlocking));
    uint8_t* H = ws->h_dsmall;
    memcpy(H + kDecSmallOffIds, ids, (size_t)n_ids * 4);
    int64_t* h_res = reinterpret_cast<int64_t*>(H + kDecSmallOffRes);
    memset(h_res, 0, 256);
    h_res[0] = -1;
    DecSmallArgs A{};
    A.h_ids = reinterpret_cast<const int32_t*>(H + kDecSmallOffIds); A.n_ids = n_ids;
    A.h_out = H + kDecSmallOffOut; A.h_result = h_res; A.utf16 = utf16 ? 1 : 0;
    A.d_bytes = utf16 ? ws->ds_bytes.as<uint8_t>() : nullptr; A.d_docbits = utf16 ? ws->ds_docbits.as<uint64_t>() : nullptr;
    TkzDecodeTable D;
    { std::lock_guard<std::mutex> lock(e->mu); D = e->D; }
    launch_dec_small(Launch{ws->st_small, nullptr, ws}, D, A);
    HIP_TRY(hipStreamSynchronize(ws->st_small));
    HIP_TRY(hipGetLastError());
    ws->dsmall_calls.fetch_add(1, std::memory_order_relaxed);
    { std::lock_guard<std::mutex> lock(e->mu); memcpy(ws->dsmall_clocks, h_res + 4, sizeof ws->dsmall_clocks); }
    if (h_res[0] < 0) return fail(TKZ_E_DEVICE, "k_dec_small left no result record");      // (the host's -1 is still there: the launch did not run to its end)
    if (h_res[0] != 0) { ws->dsmall_fallbacks.fetch_add(1, std::memory_order_relaxed); return TKZ_OK; }          // (handled stays false)
    *n_items = utf16 ? h_res[2] : h_res[1];
    *handled = true;
    return TKZ_OK;
}
tkz_status fetch_decode_small(Workspace* ws, void* out, int64_t out_cap, int64_t n_items, bool utf16) {
    if (n_items > out_cap) return fail(TKZ_E_CAPACITY, "output capacity too small");
    if (n_items) memcpy(out, ws->h_dsmall + kDecSmallOffOut, (size_t)n_items * (utf16 ? 2 : 1));
    return TKZ_OK;
}
tkz_status decode_one(tkz_encoder* e, const int32_t* ids, int64_t n_ids, void* out, int64_t out_cap, int64_t* n_out, bool utf16) {
    DeviceScope scope;
    TKZ_TRY(check_decode_one(e, scope, ids, n_ids, out, out_cap, n_out));
    if (n_ids == 0) return TKZ_OK;
    if (n_ids <= tkz::kDecSmallRouteIds && e->small_ok && !e->profiling) {
        Lease lease(e);
        bool handled = false;
        TKZ_TRY(decode_small(e, lease.ws, ids, n_ids, utf16, n_out, &handled));
        if (handled) return fetch_decode_small(lease.ws, out, out_cap, *n_out, utf16);
    }
    const int64_t id_offs[2] = {0, n_ids};
    int64_t out_offs[2] = {0, 0};
    return decode_host(e, ids, id_offs, 1, out, out_cap, out_offs, n_out, utf16);
}
}  // namespace

tkz_status tkz_decode_utf8(tkz_encoder* e, const int32_t* ids, int64_t n_ids, uint8_t* out_bytes, int64_t out_cap, int64_t* n_out) {
    return decode_one(e, ids, n_ids, out_bytes, out_cap, n_out, false);
}
tkz_status tkz_decode_utf16(tkz_encoder* e, const int32_t* ids, int64_t n_ids, uint16_t* out_units, int64_t out_cap, int64_t* n_out) {
    return decode_one(e, ids, n_ids, out_units, out_cap, n_out, true);
}
void tkz_encoder_small_decode_calls(const tkz_encoder* e, int64_t* calls, int64_t* handed_back) {
    int64_t c = 0, f = 0;
    if (e) { tkz_encoder* m = const_cast<tkz_encoder*>(e); std::lock_guard<std::mutex> lock(m->mu); for (Workspace* w : e->pool) { c += w->dsmall_calls; f += w->dsmall_fallbacks; } }
    if (calls) *calls = c;
    if (handed_back) *handed_back = f;
}
int32_t tkz_encoder_small_decode_phases(const tkz_encoder* e, int64_t* clocks16) {       // (the first workspace that has made such a call)
    if (!e || !clocks16) return 0;
    tkz_encoder* m = const_cast<tkz_encoder*>(e);
    std::lock_guard<std::mutex> lock(m->mu);
    for (Workspace* w : e->pool) if (w->h_dsmall) { memcpy(clocks16, w->dsmall_clocks, 16 * 8); return 16; }
    return 0;
}

tkz_status tkz_encoder_set_option(tkz_encoder* e, int32_t option, int64_t value) {
    if (!e) return fail(TKZ_E_ARG, "null encoder");
    if (option == TKZ_OPT_PRETOK_SEQUENTIAL) { e->pretok_seq = value != 0; return TKZ_OK; }
    if (option == TKZ_OPT_PIECE_STATS) {
        // statistics of the batch path (the single-launch path does not count): the device block is made on first use
        DeviceScope scope;
        tkz_status st = check_encoder(e, scope);
        if (st != TKZ_OK) return st;
        std::lock_guard<std::mutex> lock(e->mu);
        if (value && !e->t_stats.p) {
            HIP_TRY(e->t_stats.ensure(128, &e->bytes_allocated));        // (the block + the copy an attempt is rolled back to)
            HIP_TRY(hipMemset(e->t_stats.p, 0, 128));
        }
        e->piece_stats = value != 0;
        return TKZ_OK;
    }
    if (option == TKZ_OPT_LATENCY_BYTES) {
        if (value < 0) return fail(TKZ_E_ARG, "negative value");
        std::lock_guard<std::mutex> lock(e->mu);
        e->latency_bytes = value;
        return TKZ_OK;
    }
    if (option == TKZ_OPT_CASE_EQUIVALENCE) {
        if (value != 0 && value != 1) return fail(TKZ_E_ARG, "TKZ_OPT_CASE_EQUIVALENCE takes 0 or 1");
        std::lock_guard<std::mutex> lock(e->mu);
        e->case_equiv = value != 0;
        return TKZ_OK;
    }
    if (option == TKZ_OPT_PROMOTE_MIN_BYTES || option == TKZ_OPT_PROMOTE_CAP) {
        if (value < 0) return fail(TKZ_E_ARG, "negative value");
        std::lock_guard<std::mutex> lock(e->mu);
        if (option == TKZ_OPT_PROMOTE_MIN_BYTES) e->policy.set_min_bytes(value);
        else e->policy.set_cap((size_t)std::min<int64_t>(value, (int64_t)kPromoMaxEntries));
        return TKZ_OK;
    }
    if (option == TKZ_OPT_PROMOTE) {
        // 0 / 1: automatic promotion off / on.  2: promote NOW whatever the memo holds (every valid entry counts alike); 3: drop every promotion (the
        // key tables as the vocabulary alone gives them).  2 and 3 replace table images that a call in flight may be probing: refused unless the encoder is idle.
        DeviceScope scope;
        tkz_status st = check_encoder(e, scope);
        if (st != TKZ_OK) return st;
        if (value == 0 || value == 1) {
            { std::lock_guard<std::mutex> lock(e->mu); e->policy.set_mode((int)value); }
            if (value == 0) join_promotion(e);     // off: the tables do not change once this has returned
            return TKZ_OK;
        }
        if (value != 2 && value != 3) return fail(TKZ_E_ARG, "TKZ_OPT_PROMOTE takes 0, 1, 2 or 3");
        join_promotion(e);
        {
            std::lock_guard<std::mutex> lock(e->mu);
            for (Workspace* w : e->pool) if (w->busy) return fail(TKZ_E_ARG, "promotions can only be made or dropped by hand while no call of this encoder is in flight");
        }
        if (hipDeviceSynchronize() != hipSuccess) return fail(TKZ_E_DEVICE, "hipDeviceSynchronize");
        // (the images these two replace are RETIRED, not freed here: the check above is not held until the new ones are in place, and a call that started in
        //  between has taken its copy of the table descriptor -- the round-5 advisor; they go when no call is in flight, ~Lease)
        if (value == 2) return promote_from_memo(e, false, true, nullptr);
        { std::lock_guard<std::mutex> lock(e->mu); e->policy.reset_by_hand(); }
        return drop_promotions(e, true);      // (nothing to do when nothing is promoted)
    }
    if (option == TKZ_OPT_PIECE_MEMO) {
        // 0: off, 1: on, 2: on and emptied.  Options are set while the encoder is idle: a call in flight on another thread reads
        // T.memo_n when it launches, and emptying the table under running kernels could pair one piece's key with another's tokens
        // -- so value 2 is refused while any workspace is leased, and the device is drained before the table is cleared.
        DeviceScope scope;
        if (value == 2) join_promotion(e);     // (a promotion being built reads the memo back: not under its feet)
        std::lock_guard<std::mutex> lock(e->mu);
        if (value == 2) {
            tkz_status st = check_encoder(e, scope);
            if (st != TKZ_OK) return st;
            for (Workspace* w : e->pool) if (w->busy) return fail(TKZ_E_ARG, "the piece memo can only be emptied while no call of this encoder is in flight");
            if (hipDeviceSynchronize() != hipSuccess) return fail(TKZ_E_DEVICE, "hipDeviceSynchronize");
            if (hipMemset(e->t_memo.p, 0, size_t(e->memo_slots) * sizeof(TkzMemoSlot)) != hipSuccess) return fail(TKZ_E_DEVICE, "hipMemset");
        }
        e->T.memo_n = value ? e->memo_slots : 0u;
        return TKZ_OK;
    }
    if (option == TKZ_OPT_ADAPT) {
        if (value != 0 && value != 1) return fail(TKZ_E_ARG, "TKZ_OPT_ADAPT takes 0 or 1");
        std::lock_guard<std::mutex> lock(e->mu);
        e->policy.set_adapt((int)value);
        return TKZ_OK;
    }
    return fail(TKZ_E_ARG, "unknown option");
}

tkz_status tkz_encoder_adapt_stats(tkz_encoder* e, int64_t* out8) {
    if (!e || !out8) return fail(TKZ_E_ARG, "null argument");
    join_promotion(e);                     // (the figures after whatever is being built in the background)
    std::lock_guard<std::mutex> lock(e->mu);
    e->policy.stats(out8);
    out8[2] = (int64_t)e->promo_items.size(); out8[3] = (int64_t)e->retired.size();
    return TKZ_OK;
}

tkz_status tkz_encoder_set_profiling(tkz_encoder* e, int32_t enabled) {
    if (!e) return fail(TKZ_E_ARG, "null encoder");
    e->profiling = enabled != 0;
    return TKZ_OK;
}
tkz_status tkz_encoder_kernel_ms(tkz_encoder* e, double* ms, int64_t* launches, int32_t reset) {
    if (!e) return fail(TKZ_E_ARG, "null encoder");
    std::lock_guard<std::mutex> lock(e->mu);
    for (int k = 0; k < tkz::K_COUNT; ++k) {
        double m = 0; int64_t n = 0;
        for (Workspace* w : e->pool) { m += w->ms[k]; n += w->launches[k]; if (reset) { w->ms[k] = 0; w->launches[k] = 0; } }
        if (ms) ms[k] = m;
        if (launches) launches[k] = n;
    }
    return TKZ_OK;
}
void tkz_encoder_pretok_leftovers(const tkz_encoder* e, int64_t* after_ascii_scanner, int64_t* after_multibyte_scanner) {
    if (after_ascii_scanner) *after_ascii_scanner = e ? e->last_xcount.load() : 0;
    if (after_multibyte_scanner) *after_multibyte_scanner = e ? e->last_xcount2.load() : 0;
}
tkz_status tkz_encoder_piece_stats(tkz_encoder* e, int64_t* out8, int32_t reset) {
    if (!e || !out8) return fail(TKZ_E_ARG, "null argument");
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    join_promotion(e);                     // (the count of promoted pieces below is the one after a promotion in the background, if one is running)
    if (!e->t_stats.p) { std::lock_guard<std::mutex> lock(e->mu); out8[7] = (int64_t)e->promo_items.size(); return TKZ_OK; }
    DeviceScope scope;
    tkz_status st = check_encoder(e, scope);
    if (st != TKZ_OK) return st;
    unsigned long long h[8] = {};
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h, e->t_stats.p, sizeof h, hipMemcpyDeviceToHost));
    std::lock_guard<std::mutex> lock(e->mu);
    out8[0] = e->stat_batches; out8[1] = (int64_t)h[4]; out8[2] = (int64_t)h[2]; out8[3] = (int64_t)h[3]; out8[4] = e->stat_giants;
    out8[5] = (int64_t)h[0]; out8[6] = (int64_t)h[1]; out8[7] = (int64_t)e->promo_items.size();
    if (reset) { HIP_TRY(hipMemset(e->t_stats.p, 0, 64)); e->stat_batches = e->stat_giants = 0; }
    return TKZ_OK;
}
int64_t tkz_encoder_memo_slots(const tkz_encoder* e) { return e ? (int64_t)e->memo_slots : 0; }
void tkz_encoder_small_path_calls(const tkz_encoder* e, int64_t* calls, int64_t* handed_back) {
    int64_t c = 0, f = 0;
    if (e) { tkz_encoder* m = const_cast<tkz_encoder*>(e); std::lock_guard<std::mutex> lock(m->mu); for (Workspace* w : e->pool) { c += w->small_calls; f += w->small_fallbacks; } }
    if (calls) *calls = c;
    if (handed_back) *handed_back = f;
}
int32_t tkz_encoder_small_path_phases(const tkz_encoder* e, int64_t* clocks16) {       // shader-clock stamps of the last k_small of the first workspace
    if (!e || !clocks16) return 0;
    tkz_encoder* m = const_cast<tkz_encoder*>(e);
    std::lock_guard<std::mutex> lock(m->mu);
    for (Workspace* w : e->pool) if (w->h_small) { memcpy(clocks16, w->small_clocks, 16 * 8); return 16; }      // (a snapshot taken after the call's synchronisation, never the block a kernel may be writing)
    return 0;
}
int32_t tkz_encoder_memo_ways(const tkz_encoder* e) { return e ? (int32_t)kMemoWays : 0; }
int64_t tkz_encoder_memo_bucket(const tkz_encoder* e, const uint8_t* piece, int32_t len) {
    if (!e || !piece || len < 1 || len > 16 || !e->memo_slots) return -1;
    uint32_t kw[4] = {0, 0, 0, 0};
    for (int32_t i = 0; i < len; ++i) { if (!piece[i]) return -1; kw[i >> 2] |= (uint32_t)piece[i] << (8 * (i & 3)); }      // (pieces with a zero byte never use the memo)
    return (int64_t)tkz_mulhi(tkz_hash_memo(kw, (uint32_t)len), e->memo_slots / kMemoWays);
}
// CreateTokenizer is where a drop-in pays construction costs (TokenizerBuilder.cs:210-213), not the first Encode: the workspace of a batch of up to
// max_bytes bytes in max_docs documents -- ~7.8 bytes per input byte -- is allocated here instead of inside the first batch call, where its hipMallocs
// took anything from 5 ms to seconds.  Later batches of up to that size allocate nothing (lists that a miss-heavy text needs longer still grow once).
tkz_status tkz_encoder_reserve(tkz_encoder* e, int64_t max_bytes, int64_t max_docs) {
    using namespace tkz;
    if (!e) return fail(TKZ_E_ARG, "null encoder");
    if (max_bytes < 0 || max_docs < 0) return fail(TKZ_E_ARG, "negative size");
    DeviceScope scope;
    tkz_status st = check_encoder(e, scope);
    if (st != TKZ_OK) return st;
    Lease lease(e);
    Workspace* ws = lease.ws;
    int64_t* acc = &ws->bytes_allocated;
    st = prepare_workspace(ws, max_bytes, max_docs, CallKind::Encode);
    if (st != TKZ_OK) return st;
    const int64_t nwords = max_bytes / 64 + 1;
    HIP_TRY(ws->w_xq.ensure((size_t)(nwords / kRowsPerWave + 4) * 16, acc));                      // (the o200k scanners' queues)
    {   // (an encoder with special tokens registered: the special entries' bitmaps)
        bool lits; { std::lock_guard<std::mutex> lock(e->mu); lits = e->lit_state == 1; }
        if (lits) for (DevBuf* b : {&ws->w_candbits, &ws->w_segbits, &ws->w_specbits, &ws->w_endbits}) HIP_TRY(b->ensure((size_t)(nwords + 8) * 8, acc));
    }
    if (!ws->h_counters) HIP_TRY(hipHostMalloc((void**)&ws->h_counters, sizeof(CounterBlock), 0));
    HIP_TRY(ensure_streams(ws));
    {   // what the host-buffer entry points stage a chunk in (two input sets, three output sets: encode_host cuts a large batch into chunks of at most 32 MB; the
        // second workspace its pipeline leases for every other chunk is a chunk's size and sizes itself on its first use)
        const int64_t chunk = std::min<int64_t>(max_bytes, int64_t(32) << 20), cdocs = std::min<int64_t>(max_docs, std::max<int64_t>(1, chunk / 16));
        for (int q = 0; q < 3; ++q) {
            if (q < 2) {
                HIP_TRY(ws->s_bytes[q].ensure((size_t)chunk + 64, acc));
                HIP_TRY(ws->s_offs[q].ensure((size_t)(cdocs + 1) * 8, acc));
            }
            HIP_TRY(ws->s_out[q].ensure((size_t)std::max<int64_t>(chunk, 1) * 4, acc));
            HIP_TRY(ws->s_outoffs[q].ensure((size_t)(cdocs + 1) * 8, acc));
        }
    }
    {   // the counters and the log of a learning window (TKZ_OPT_PROMOTE)
        std::lock_guard<std::mutex> lock(e->mu);
        if (e->memo_slots && e->policy.mode() == 1) {
            if (e->t_memo_hits.ensure((size_t)e->memo_slots * 4, &e->bytes_allocated) != hipSuccess ||
                e->t_long_log.ensure((size_t)kLongLogCap * kLongLogDwords * 4 + 64, &e->bytes_allocated) != hipSuccess)
                return fail(TKZ_E_OUT_OF_MEMORY, "learning buffers could not be allocated");
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    return TKZ_OK;
}
int64_t tkz_encoder_workspace_bytes(const tkz_encoder* e) {
    if (!e) return 0;
    tkz_encoder* m = const_cast<tkz_encoder*>(e);
    std::lock_guard<std::mutex> lock(m->mu);
    int64_t n = e->bytes_allocated;
    for (Workspace* w : e->pool) n += w->bytes_allocated;
    return n;
}
int64_t tkz_encoder_side_by_side_batches(const tkz_encoder* e) {
    if (!e) return 0;
    tkz_encoder* m = const_cast<tkz_encoder*>(e);
    std::lock_guard<std::mutex> lock(m->mu);
    int64_t n = 0;
    for (Workspace* w : e->pool) n += w->forked_batches;
    return n;
}
int64_t tkz_encoder_engine_downloads(const tkz_encoder* e) {
    if (!e) return 0;
    tkz_encoder* m = const_cast<tkz_encoder*>(e);
    std::lock_guard<std::mutex> lock(m->mu);
    int64_t n = 0;
    for (Workspace* w : e->pool) n += w->engine_downloads.load(std::memory_order_relaxed);
    return n;
}
const char* tkz_kernel_name(int32_t k) {
    static const char* const names[] = {"k_docmark", "k_pretok", "k_probe", "k_scan", "k_place", "k_docoffs", "k_merge_long_group", "k_merge_short"};
    return (k >= 0 && k < tkz::K_COUNT) ? names[k] : "?";
}

tkz_status tkz_corpus_generate_device(int32_t device, int32_t kind, uint64_t seed, int64_t first_doc, int64_t n_docs,
                                      int32_t min_len, int32_t max_len, int64_t* d_doc_offsets, uint8_t* d_bytes,
                                      int64_t cap_bytes, void* hip_stream, int64_t* total_bytes) {
    if (kind < 1 || kind > 5 || kind == 4 || n_docs < 0 || min_len < 0 || max_len < min_len || !d_doc_offsets || !total_bytes)
        return fail(TKZ_E_ARG, "bad corpus arguments");
    DeviceScope scope;
    hipError_t r = scope.enter(device);
    if (r != hipSuccess) return fail(TKZ_E_NO_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(r));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    int64_t* d_total = nullptr;
    HIP_TRY(hipMalloc((void**)&d_total, 8));
    tkz::launch_corpus(s, kind, seed, first_doc, n_docs, min_len, max_len, d_doc_offsets, d_bytes, d_bytes ? cap_bytes : 0, d_total);
    hipError_t c = hipMemcpyAsync(total_bytes, d_total, 8, hipMemcpyDeviceToHost, s);
    if (c == hipSuccess) c = hipStreamSynchronize(s);
    if (c == hipSuccess) c = hipGetLastError();
    (void)hipFree(d_total);
    if (c != hipSuccess) return fail(TKZ_E_DEVICE, std::string("corpus generation: ") + hipGetErrorString(c));
    if (d_bytes && *total_bytes > cap_bytes) return fail(TKZ_E_CAPACITY, "corpus buffer too small");
    return TKZ_OK;
}

// ---- shard arithmetic of the multi-GPU partitioning (the communicator itself is tkz_comm.cpp) ----
void tkz_shard_range(int64_t n_docs_total, int32_t rank, int32_t world, int64_t* lo, int64_t* hi) {
    if (world < 1) world = 1;
    // (128-bit product: n_docs_total * world may exceed 2^63 only for absurd inputs, but costs nothing to get right)
    if (lo) *lo = (int64_t)(((__int128)n_docs_total * rank) / world);
    if (hi) *hi = (int64_t)(((__int128)n_docs_total * (rank + 1)) / world);
}

tkz_status tkz_shard_bases(const int64_t* table, int32_t world, int32_t rank, int64_t* bases3, int64_t* totals3) {
    if (!table || world < 1 || rank < 0 || rank >= world) return fail(TKZ_E_ARG, "bad table / rank");
    int64_t b[3] = {0, 0, 0}, t[3] = {0, 0, 0};
    for (int r = 0; r < world; ++r)
        for (int k = 0; k < 3; ++k) {
            const int64_t v = table[3 * r + k];
            if (v < 0) return fail(TKZ_E_ARG, "negative count in the gathered table");
            if (r < rank) b[k] += v;
            t[k] += v;
        }
    if (bases3) memcpy(bases3, b, sizeof b);
    if (totals3) memcpy(totals3, t, sizeof t);
    return TKZ_OK;
}

int64_t tkz_corpus_generate_doc_host(int32_t kind, uint64_t seed, int64_t doc_index, int32_t min_len, int32_t max_len,
                                     uint8_t* buf, int64_t cap) {
    if (kind < 1 || kind > 5 || kind == 4 || min_len < 0 || max_len < min_len) return -1;
    return tkz_corpus_doc(kind, seed, doc_index, min_len, max_len, buf, cap);
}

}  // extern "C"
