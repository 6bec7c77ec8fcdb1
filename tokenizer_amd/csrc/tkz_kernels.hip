// tkz_kernels.hip -- the HIP kernels of the batch encode path, written for gfx950 (wave64, 256-thread
// workgroups, LDS-staged tiles) and their launchers.
//
// Pipeline for one batch of documents already resident in HBM (bytes = all documents back to back,
// offs[d] = first byte of document d):
//
//   k_docmark        doc offsets -> 1 bit per byte "a document starts here" (+ a sentinel bit at `total`)
//   k_pretok_rows    Regex.Matches for pattern 1 / cl100k, position-parallel (tkz_pretok.h (2))
//   k_pretok_seq     Regex.Matches for any pattern, one lane per document (tkz_pretok.h (1))
//                    -> 1 bit per byte "a piece starts here"
//   k_doccount2/scan documents and pieces that start in each 1 KiB sub-tile -> ordinal bases
//   k_probe          per sub-tile, one wavefront: enumerate pieces from the bitmap, whole-piece lookup
//                    (TikTokenizer.cs:262) -> one 32-bit record per piece
//   k_merge_short    BytePairEncode (BytePairEncoder.cs:13-76) of the missed pieces of <= 16 bytes, 64 per wavefront
//   k_giant_* / k_merge_coop   the missed pieces of > 1024 bytes (a workgroup each) / of 129..1024 bytes (a wavefront each)
//   k_long_count / k_long_scatter / k_merge_long_q   the missed pieces of 17..128 bytes of a LARGE batch, a lane each: binned by length class across the
//                    whole batch, then merged off that queue 64 of one class at a time (k_merge_long: the same batches formed inside a unit of a few
//                    sub-tiles -- a small batch, and the single-launch kernel)
//   k_scan_*         exclusive scan of the per-sub-tile token counts
//   k_place          ids stored at their final position
//   k_docoffs        out_offsets[d] = tile base + position inside the tile
#include "tkz_kernels.h"

#include <type_traits>

#include "tkz_bpe.h"
#include "tkz_classes.h"
#include "tkz_corpus.h"
#include "tkz_pretok.h"
#include "tkz_simt.h"

namespace tkz {

// -------------------------------------------------------------------------------------------------
// k_docmark
// -------------------------------------------------------------------------------------------------
// has_empty: null, or a word that is set when an item is empty (offs[d] == offs[d + 1]): k_docoffs then looks every mark's ordinal up, and takes the
// item's index for it otherwise.  (A plain store of the same 1 by every lane that sees one: an atomic per empty document would serialise a batch of a
// million of them on one line, as k_probe's REPORT once did.)
TKZ_KERNEL(256) void k_docmark(const int64_t* offs, int64_t n_items, int64_t total, uint64_t* bits, int32_t* counters, int32_t* has_empty) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d <= n_items; d += stride) {
        const int64_t pos = offs[d];
        bool ok = pos >= 0 && pos <= total;
        if (d == 0) ok = ok && pos == 0;
        if (d == n_items) ok = ok && pos == total;
        else {
            const int64_t next = offs[d + 1];
            ok = ok && pos <= next;
            if (has_empty && pos == next) *has_empty = 1;
        }
        if (!ok) { simt::atomic_or((unsigned*)&counters[0], (unsigned)kErrOffsets); continue; }
        // One plain store per bitmap word, by the first item that starts in it (the words were zeroed; 10 M atomics were a read-modify-write of nearly every
        // line of a 640 MB bitmap).  Offsets that are not monotone are reported by the item that sees it and the batch fails: what is stored then is never used.
        const int64_t w = pos >> 6;
        if (d > 0) { const int64_t prev = offs[d - 1]; if (prev >= 0 && prev <= pos && (prev >> 6) == w) continue; }
        uint64_t m = 1ull << (pos & 63);
        int64_t cur = pos;
        for (int64_t e = d + 1; e <= n_items;) {
            const int64_t q = offs[e];
            if (q < cur || (q >> 6) != w) break;
            if (q == cur) {                                // a run of empty documents: to its end by bisection (a million of them are 20 steps, not a million)
                int64_t lo = e + 1, hi = n_items + 1;
                while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (offs[mid] <= cur) lo = mid + 1; else hi = mid; }
                e = lo;
                continue;
            }
            m |= 1ull << (q & 63);
            cur = q; ++e;
        }
        bits[w] = m;
    }
}

// -------------------------------------------------------------------------------------------------
// k_pretok_rows : one wave per kRowsPerWave rows of 64 bytes
// -------------------------------------------------------------------------------------------------
// classification of one row: general (any UTF-8) or, when its 64 bytes are all ASCII, from the flag table
struct RowInfo { TkzRowLane L; TkzRowMasks m; bool simple; };
template <int PATTERN>
TKZ_DEV RowInfo tkz_load_row(const TkzSrc& S, int64_t row, const uint8_t* bmp, const uint16_t* aflags) {
    RowInfo r;
    const int64_t pos = (row << 6) + simt::lane();
    const uint32_t b = tkz_gbyte(S, pos);
    const bool full = row >= 0 && ((row + 1) << 6) <= S.total;
    r.simple = full && simt::ballot(b >= 0x80u) == 0;
    if (r.simple) {
        const uint32_t f = aflags[b];
        r.L.pc = tkz_pc_of_flags(f); r.L.len = 1; r.L.off = 0; r.L.b = b; r.L.bad = 0;
        r.m = tkz_row_masks_ascii(f);
    } else {
        r.L = tkz_classify_byte(S, pos, bmp);
        r.m = tkz_row_masks(r.L, PATTERN == TKZ_PAT_CL100K);
    }
    return r;
}

// The sequential row loop over rows [r0, r1): rows one after the other, scan state carried in scalars.
template <int PATTERN>
TKZ_DEV void tkz_rows_sequential(const TkzSrc& S, const uint64_t* docbits, uint64_t* startbits, int64_t nrows, const uint8_t* bmp,
                                 const uint16_t* aflags, int64_t r0, int64_t r1, int32_t* counters) {
    const int lane = simt::lane();
    auto ds_at = [&](int64_t r) -> uint64_t { return (r >= 0 && r < nrows) ? docbits[r] : 0; };
    // warm-up start: the nearest row boundary at or before r0 across which no scan state flows
    // (the byte before it is neither a digit nor CR/LF, or a document starts exactly there)
    int64_t rw = r0;
    while (rw > 0) {
        if (ds_at(rw) & 1ull) break;
        // (first_lane: every lane looks at the same byte, but the compiler only knows that if told -- a lane-varying
        //  `rw` would drag every mask of the row loop from the scalar unit onto the VALU)
        const int pc = simt::first_lane(tkz_classify_byte(S, (rw << 6) - 1, bmp).pc);
        if (pc != PC_N && pc != PC_CRLF) break;
        --rw;
    }
    TkzScanCarry cy;
    cy.nb63 = 0; cy.carryN = 0; cy.abs63 = 0; cy.sa_from = -1; cy.sa_end = -1; cy.sa_lastcr = -1;
    int64_t row = rw > 0 ? rw - 1 : 0;                     // one extra row so the flags carried from "previous" are real
    RowInfo P = tkz_load_row<PATTERN>(S, row - 1, bmp, aflags);
    RowInfo C = tkz_load_row<PATTERN>(S, row, bmp, aflags);
    uint64_t dsP = ds_at(row - 1), dsC = ds_at(row);
    int clenP = 0, o1msP = 0, bad = 0;
    uint64_t c2P = 0, c3P = 0, o1P = 0;
    for (; row < r1; ++row) {
        const RowInfo N = tkz_load_row<PATTERN>(S, row + 1, bmp, aflags);
        const uint64_t dsN = ds_at(row + 1);
        int clenC, o1msC;
        uint64_t c2C, c3C, o1C, out;
        if (C.simple && N.simple) {
            out = tkz_row_eval_ascii<PATTERN>(P.m, C.m, N.m, dsC, dsN, c2P, c3P, o1P, &c2C, &c3C, &o1C, cy, S, docbits, nrows, bmp, row);
            clenC = (int)((c2C >> lane) & 1ull) * 2 + (int)((c3C >> lane) & 1ull) * 3;
            o1msC = (int)((o1C >> lane) & 1ull);
        } else {
            out = tkz_row_eval<PATTERN>(P.L, C.L, N.L, dsP, dsC, dsN, C.m, N.m, clenP, o1msP, &clenC, &o1msC, &c2C, &c3C, &o1C, cy,
                                        S, docbits, nrows, bmp, row);
        }
        if (row >= r0) {
            if (lane == 0) startbits[row] = out;
            bad |= C.L.bad | ((C.L.off != 0 && ((dsC >> lane) & 1ull)) ? 1 : 0);   // a document may not start inside a char
        }
        P = C; C = N; dsP = dsC; dsC = dsN; clenP = clenC; o1msP = o1msC; c2P = c2C; c3P = c3C; o1P = o1C;
    }
    if (simt::ballot(bad != 0) && lane == 0) simt::atomic_or((unsigned*)&counters[0], (unsigned)kErrUtf8);
}

// The 4 KiB of a block (rows first .. first+63: 16-byte chunk c = lane + 64 q is part c%4 of row c/4) and the first 16 bytes of the row behind it (a char of
// the last row may end there), requested TOGETHER: four named requests and the trailing one per lane, nothing waited for in between -- one round trip to the
// memory, where a rolled loop (request, wait, LDS write, four times) and a scalar load of the trailing row made five.  Every staged row is a full row of the
// corpus (`inside`, the caller's), so a chunk in front of the corpus (block 0: pos < 0) and the lanes that have no trailing row to fetch read the block's
// first bytes instead -- a line the wavefront requests anyway -- and drop them: no request sits inside a branch, and none is uniform (a uniform one goes
// through the scalar cache and is waited for on its own).
struct PretokStage { uint4 v0, v1, v2, v3, z; };
TKZ_DEV uint4 tkz_load16_or_zero(const uint8_t* bytes, int64_t pos, int64_t safe, bool ok) {
    uint4 v = tkz_load16(bytes + (ok ? pos : safe));
    if (!ok) v.x = v.y = v.z = v.w = 0;
    return v;
}
TKZ_DEV void tkz_pretok_request(const uint8_t* bytes, int64_t total, int64_t first, PretokStage& st) {
    const int lane = simt::lane();
    const int64_t safe = first < 0 ? 0 : first << 6;
    const int64_t p0 = (first << 6) + 16 * (int64_t)lane, p1 = p0 + 1024, p2 = p0 + 2048, p3 = p0 + 3072;
    const int64_t tpos = (first + 64) << 6;
    st.v0 = tkz_load16_or_zero(bytes, p0, safe, p0 >= 0);
    st.v1 = tkz_load16_or_zero(bytes, p1, safe, p1 >= 0);
    st.v2 = tkz_load16_or_zero(bytes, p2, safe, p2 >= 0);
    st.v3 = tkz_load16_or_zero(bytes, p3, safe, p3 >= 0);
    st.z = tkz_load16_or_zero(bytes, tpos, safe, lane == 0 && tpos + 16 <= total);
}
TKZ_DEV void tkz_pretok_fill(uint4* s_blk, const PretokStage& st) {
    const int lane = simt::lane();
    uint4* const at = s_blk + ((lane >> 2) * kBlockRowStride + (lane & 3) * 16) / 16;       // chunk c = lane; chunk c + 64 is 16 rows further on
    at[0] = st.v0; at[kBlockRowStride] = st.v1; at[2 * kBlockRowStride] = st.v2; at[3 * kBlockRowStride] = st.v3;
    if (lane < kBlockRowStride / 16) s_blk[(64 * kBlockRowStride) / 16 + lane] = st.z;      // (lane 0: the trailing row's bytes; zeros beyond)
}

template <int PATTERN>
TKZ_KERNEL(64) void k_pretok_rows(const uint8_t* bytes, int64_t total, const uint64_t* docbits, uint64_t* startbits,
                                  int64_t nrows, const uint8_t* bmp, int32_t* counters, int64_t* xq, unsigned long long* xcount) {
    // One wavefront per workgroup (the chunk index is then blockIdx.x, which the compiler knows to be wave-uniform).
    // The wavefront owns output rows [r0, r0 + kRowsPerWave); it stages rows r0-1 .. r0+62 (one per lane) in LDS and
    // evaluates them all at once (tkz_block_eval); blocks that scheme refuses go through the sequential row loop.
    TKZ_SHARED uint16_t s_aflags[128];
    TKZ_SHARED uint4 s_blk[(65 * kBlockRowStride) / 16];
    const int lane = simt::lane();
    const int64_t r0 = simt::bid() * kRowsPerWave;
    const int64_t first = r0 - 1;                          // row of lane 0
    const bool inside = ((first + 64) << 6) <= total;       // every staged row is a full row of the corpus
    if (inside) {
        // the block, the row behind it and this lane's word of document marks: all requested before the first wait
        const int64_t row = first + lane;
        uint64_t ds = 0;
        PretokStage st;
        tkz_pretok_request(bytes, total, first, st);
        if (row >= 0 && row < nrows) ds = docbits[row];
        tkz_pretok_fill(s_blk, st);
        simt::sync();
        if (r0 >= nrows) return;
        uint64_t out;
        bool done;
        if constexpr (PATTERN == TKZ_PAT_O200K) {
            TkzBlockCtx X; X.bytes = bytes; X.docbits = docbits; X.total = total; X.nrows = nrows; X.row0 = first;
            done = tkz_block_eval_o200k(reinterpret_cast<const uint8_t*>(s_blk), ds, X, &out);
        } else done = tkz_block_eval<PATTERN>(reinterpret_cast<const uint8_t*>(s_blk), ds, bmp, &out);
        if (done) {
            if (lane >= 1 && lane <= kRowsPerWave && row < nrows) startbits[row] = out;
            if (PATTERN == TKZ_PAT_O200K && lane == 0) reinterpret_cast<uint8_t*>(xq)[simt::bid()] = 0;
            return;
        }
    } else if (r0 >= nrows) return;                        // (`inside` is the same for the whole workgroup -- one wavefront -- so every lane meets the same barriers)
    const int64_t r1 = r0 + kRowsPerWave < nrows ? r0 + kRowsPerWave : nrows;
    if constexpr (PATTERN == TKZ_PAT_O200K) {
        // no row-sequential scanner for o200k: the block's rows start as the document-start bits and the block goes to
        // k_pretok_seq_blocks (sequential matcher from the nearest guaranteed match start)
        // (a flag per block, not a queue: one queue counter serialises a quarter of a million atomics per GB of non-ASCII text)
        for (int64_t r = r0 + lane; r < r1; r += 64) startbits[r] = docbits[r];
        if (lane == 0) reinterpret_cast<uint8_t*>(xq)[simt::bid()] = 1;
    } else {
        // the per-byte flag table is read by the row loop only: filled here, behind the block evaluator's refusal
        for (int i = lane; i < 128; i += 64) s_aflags[i] = (uint16_t)tkz_ascii_flags((uint32_t)i, PATTERN == TKZ_PAT_CL100K);
        simt::sync();
        TkzSrc S;
        S.bytes = bytes; S.total = total; S.stage = nullptr; S.lo = 0; S.hi = 0;
        tkz_rows_sequential<PATTERN>(S, docbits, startbits, nrows, bmp, s_aflags, r0, r1, counters);
    }
}

// The same for ONE block by ONE wavefront of a larger workgroup (k_small): pattern 1 / cl100k only, wavefront-level synchronisation only.
constexpr int kPretokBlkQuads = (65 * kBlockRowStride) / 16;
template <int PATTERN>
TKZ_DEV void tkz_pretok_block(int64_t blk, uint4* s_blk, const uint16_t* s_aflags, const uint8_t* bytes, int64_t total, const uint64_t* docbits,
                              uint64_t* startbits, int64_t nrows, const uint8_t* bmp, int32_t* counters) {
    static_assert(PATTERN != TKZ_PAT_O200K, "o200k blocks need the two follow-up kernels");
    const int lane = simt::lane();
    const int64_t r0 = blk * kRowsPerWave;
    if (r0 >= nrows) return;
    const int64_t first = r0 - 1;                          // row of lane 0
    const bool inside = ((first + 64) << 6) <= total;       // every staged row is a full row of the corpus
    if (inside) {
        (void)simt::ballot(true);                          // (the block before this one is no longer read)
        const int64_t row = first + lane;
        uint64_t ds = 0;
        PretokStage st;
        tkz_pretok_request(bytes, total, first, st);       // (as in k_pretok_rows: every request before the first wait)
        if (row >= 0 && row < nrows) ds = docbits[row];
        tkz_pretok_fill(s_blk, st);
        (void)simt::ballot(true);
        uint64_t out;
        if (tkz_block_eval<PATTERN>(reinterpret_cast<const uint8_t*>(s_blk), ds, bmp, &out)) {
            if (lane >= 1 && lane <= kRowsPerWave && row < nrows) startbits[row] = out;
            return;
        }
    }
    const int64_t r1 = r0 + kRowsPerWave < nrows ? r0 + kRowsPerWave : nrows;
    TkzSrc S;
    S.bytes = bytes; S.total = total; S.stage = nullptr; S.lo = 0; S.hi = 0;
    tkz_rows_sequential<PATTERN>(S, docbits, startbits, nrows, bmp, s_aflags, r0, r1, counters);
}

// o200k, second pass: the blocks k_pretok_rows<O200K> left over because they hold multi-byte chars, through the char-level block
// evaluator (tkz_block_eval_o200k_mb).  A kernel of its own so that its registers stay out of the ASCII scanner's.  What it
// refuses as well goes into the second queue, for k_pretok_seq_blocks.
TKZ_KERNEL_OCC(64, 3) void k_pretok_mb_blocks(const uint8_t* bytes, int64_t total, const uint64_t* docbits, uint64_t* startbits, int64_t nrows,
                                       const uint8_t* bmp, const uint8_t* xflag, int64_t nblk, unsigned long long* xcount, int64_t* xq2, unsigned long long* xcount2,
                                       int by_code_point) {
    TKZ_SHARED uint4 s_blk[(65 * kBlockRowStride) / 16];
    const int lane = simt::lane();
    unsigned long long mine = 0;
    for (int64_t blk = simt::bid(); blk < nblk; blk += simt::nblocks()) {
        if (xflag[blk] != 1) continue;                         // (one wavefront per workgroup: the branch is uniform)
        ++mine;
        const int64_t r0 = blk * kRowsPerWave, first = r0 - 1;
        bool done = false;
        uint64_t out = 0;
        simt::sync();                                          // (the previous block's rows are no longer read)
        // rows first .. first+63 and the first 16 bytes of the row behind them; what lies outside the corpus reads as 0 -- the
        // sentinel bit at `total` makes whatever follows the last document a document of its own, so the padding changes nothing
        // (five named requests a lane -- chunk c = lane + 64 q, the fifth by lanes 0..3 -- and the lane's word of document marks, all in front of the first
        //  wait; the chunk the corpus ends in is rare and is put together byte by byte behind them)
        const int64_t row = first + lane;
        uint64_t ds = 0;
        auto request = [&](int q) -> uint4 {                   // chunk c = lane + 64 q where the corpus holds all 16 bytes of it, zeros elsewhere
            const int c = lane + 64 * q;
            const int64_t pos = (first << 6) + 16 * (int64_t)c;
            uint4 v; v.x = v.y = v.z = v.w = 0;
            if (c < 260 && pos >= 0 && pos + 16 <= total) v = tkz_load16(bytes + pos);
            return v;
        };
        auto fill = [&](int q, uint4 v) {
            const int c = lane + 64 * q;
            const int64_t pos = (first << 6) + 16 * (int64_t)c;
            if (c < 260 && pos >= 0 && pos + 16 > total && pos < total) {
                uint32_t w[4] = {0, 0, 0, 0};
                for (int j = 0; j < 16; ++j) if (pos + j < total) w[j >> 2] |= (uint32_t)bytes[pos + j] << (8 * (j & 3));
                v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
            }
            if (c < 256) s_blk[((c >> 2) * kBlockRowStride + (c & 3) * 16) / 16] = v;
            else if (c < 260) {
                if (c != 256) v.x = v.y = v.z = v.w = 0;
                s_blk[(64 * kBlockRowStride) / 16 + (c - 256)] = v;
            }
        };
        const uint4 v0 = request(0), v1 = request(1), v2 = request(2), v3 = request(3), v4 = request(4);
        if (row >= 0 && row < nrows) ds = docbits[row];
        fill(0, v0); fill(1, v1); fill(2, v2); fill(3, v3); fill(4, v4);
        if (lane == 0) { uint4 z; z.x = z.y = z.z = z.w = 0; s_blk[(64 * kBlockRowStride) / 16 + 4] = z; }
        simt::sync();
        {
            TkzBlockCtx X; X.bytes = bytes; X.docbits = docbits; X.total = total; X.nrows = nrows; X.row0 = first;
            done = tkz_block_eval_o200k_mb(reinterpret_cast<const uint8_t*>(s_blk), ds, X, bmp, by_code_point != 0, &out);
            if (done && lane >= 1 && lane <= kRowsPerWave && row < nrows) startbits[row] = out;
        }
        if (!done && lane == 0) xq2[simt::atomic_add64(xcount2, 1ull)] = blk;
    }
    if (mine && lane == 0) simt::atomic_add64(xcount, mine);    // (statistics: tkz_encoder_pretok_leftovers)
}

// one document through the sequential matcher from match start p0; piece starts inside [b0, b1) are OR-ed into startbits
TKZ_DEV void tkz_seq_emit(int pattern, const TkzDoc& doc, int64_t a, int64_t p0, int64_t b0, int64_t b1, uint64_t* startbits) {
    int64_t curw = -1; uint64_t acc = 0;
    for (int64_t p = p0; p < doc.n && a + p < b1;) {
        const int64_t g = a + p;
        if (g >= b0) {
            if ((g >> 6) != curw) {
                if (acc) simt::atomic_or64((unsigned long long*)&startbits[curw], acc);
                curw = g >> 6; acc = 0;
            }
            acc |= 1ull << (g & 63);
        }
        p = tkz_match_at(pattern, doc, p);
    }
    if (acc) simt::atomic_or64((unsigned long long*)&startbits[curw], acc);
}

constexpr int kSeqBack = 768, kSeqFwd = 384, kSeqSeg = 62, kSeqWin = kSeqBack + kRowsPerWave * 64 + kSeqFwd;
static_assert(kSeqSeg * 64 == kRowsPerWave * 64 && kSeqWin % 16 == 0, "64 segments tile a block");
// byte i is certainly a match start when (byte i-1, byte i) are: CR/LF then an ASCII letter or digit; a non-white-space ASCII char then an
// ASCII white-space char that is not CR/LF; a non-digit ASCII char then an ASCII digit (no alternative of the patterns spans any of these)
TKZ_HD bool tkz_sync_rule(uint32_t pc, uint32_t c) {
    if (pc >= 0x80u || c >= 0x80u) return false;
    const bool c_ws = c == ' ' || c - 9u < 5u, pc_ws = pc == ' ' || pc - 9u < 5u;
    if ((pc == '\n' || pc == '\r') && ((c | 0x20u) - 'a' < 26u || c - '0' < 10u)) return true;
    if (c_ws && c != '\n' && c != '\r' && !pc_ws) return true;
    return c - '0' < 10u && !(pc - '0' < 10u);
}
// one block through the sequential matcher straight from HBM, by ONE lane: every document that overlaps [b0, b1) from the nearest sync
// point at or before b0
TKZ_DEV void tkz_seq_block_global(const uint8_t* bytes, const int64_t* offs, int64_t n_docs, int64_t total, uint64_t* startbits, int pattern,
                                  const uint8_t* bmp, int64_t b0, int64_t b1, int32_t* counters) {
    int64_t lo = 0, hi = n_docs;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (offs[mid + 1] <= b0) lo = mid + 1; else hi = mid; }
    for (int64_t d = lo; d < n_docs && offs[d] < b1; ++d) {
        const int64_t a = offs[d], e = offs[d + 1];
        if (e <= a || a < 0 || e > total) continue;
        TkzDoc doc; doc.b = bytes + a; doc.n = e - a; doc.bmp = bmp; doc.by_code_point = pattern == TKZ_PAT_O200K;
        int64_t p = 0;
        if (a < b0) {
            int64_t i = b0 - a;
            for (; i > 0; --i) if (tkz_sync_rule(doc.b[i - 1], doc.b[i])) break;
            p = i;
        }
        int bad = 0;
        int64_t v = a < b0 ? b0 - a : 0;                    // validate from the start of the char that contains the block's first byte
        for (int back = 0; v > 0 && back < 3 && (doc.b[v] & 0xC0) == 0x80; ++back) --v;
        for (; v < doc.n && a + v < b1;) { const TkzChar ch = tkz_doc_char(doc, v); bad |= ch.bad; v += ch.len; }
        if (bad) { simt::atomic_or((unsigned*)&counters[0], (unsigned)kErrUtf8); continue; }
        tkz_seq_emit(pattern, doc, a, p, b0, b1, startbits);
    }
}

// The blocks k_pretok_rows<O200K> left over.  For every document that overlaps the block's
// bytes the sequential matcher runs from the nearest position at or before the block that is certainly a match start --
// the document start; a letter/digit right after a CR/LF; an ASCII non-CR/LF white-space char after a non-white-space
// ASCII char; an ASCII digit after a non-digit ASCII char (no alternative of the pattern can span any of these) -- and
// the piece starts that fall inside the block are OR-ed in (one wavefront per block).  When more than a quarter of all blocks were left over
// (text that is mostly non-ASCII) the kernel instead runs one lane per DOCUMENT over the whole batch: OR-ing the bits
// of blocks that were already done is harmless.
TKZ_KERNEL(256) void k_pretok_seq_blocks(const uint8_t* bytes, const int64_t* offs, int64_t n_docs, int64_t total, uint64_t* startbits,
                                         int64_t nrows, int pattern, const uint8_t* bmp, const int64_t* xq, const unsigned long long* xcount,
                                         int32_t* counters) {
    const int64_t nx = (int64_t)*xcount;
    const int64_t nblk = (nrows + kRowsPerWave - 1) / kRowsPerWave;
    const int64_t stride = simt::nblocks() * simt::nthreads();
    if (nx * 4 > nblk) {
        for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d < n_docs; d += stride) {
            const int64_t a = offs[d], e = offs[d + 1];
            if (e <= a || a < 0 || e > total) continue;
            TkzDoc doc; doc.b = bytes + a; doc.n = e - a; doc.bmp = bmp; doc.by_code_point = pattern == TKZ_PAT_O200K;
            int bad = 0;
            for (int64_t v = 0; v < doc.n;) { const TkzChar ch = tkz_doc_char(doc, v); bad |= ch.bad; v += ch.len; }
            if (bad) { simt::atomic_or((unsigned*)&counters[0], (unsigned)kErrUtf8); continue; }
            tkz_seq_emit(pattern, doc, a, 0, a, e, startbits);
        }
        return;
    }
    // One WAVEFRONT per block.  The block (+ 768 bytes before it, 384 after) is staged in LDS -- the matcher reads a char at a time,
    // every read a dependent round trip when it goes to HBM: a lane took ~1 us per byte that way -- and cut into 64 segments of 62
    // bytes at sync points: lane l matches from the first sync point at or after the start of its segment up to the one lane l+1
    // starts from (lane 0: from the nearest sync point before the block).  When the window holds no sync point where one is needed
    // (text without blanks, digits or line breaks for hundreds of bytes) lane 0 does the block from HBM, as before.
    TKZ_SHARED uint4 s_win_all[kThreads / 64][kSeqWin / 16];
    uint8_t* const win = reinterpret_cast<uint8_t*>(s_win_all[simt::wave()]);
    const int lane = simt::lane();
    for (int64_t q = (simt::bid() * simt::nthreads() + simt::tid()) >> 6; q < nx; q += stride >> 6) {
        const int64_t r0 = xq[q] * kRowsPerWave;
        const int64_t r1 = r0 + kRowsPerWave < nrows ? r0 + kRowsPerWave : nrows;
        const int64_t b0 = r0 << 6, b1 = (r1 << 6) < total ? (r1 << 6) : total;
        if (b0 >= b1) continue;
        const int64_t wlo = b0 > kSeqBack ? b0 - kSeqBack : 0;             // (multiples of 64)
        const int64_t whi = b1 + kSeqFwd < total ? b1 + kSeqFwd : total;
        (void)simt::ballot(true);                                           // (the previous block's window is no longer read)
        for (int64_t p = wlo + 16 * lane; p < whi; p += 16 * 64) {
            uint4 v; v.x = v.y = v.z = v.w = 0;
            if (p + 16 <= total) v = tkz_load16(bytes + p);
            else {
                uint32_t w[4] = {0, 0, 0, 0};
                for (int k = 0; k < 16; ++k) if (p + k < total) w[k >> 2] |= (uint32_t)bytes[p + k] << (8 * (k & 3));
                v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
            }
            *reinterpret_cast<uint4*>(win + (p - wlo)) = v;
        }
        (void)simt::ballot(true);
        auto wb = [&](int64_t abs) -> uint32_t { return win[abs - wlo]; };
        auto doc_of = [&](int64_t pos) -> int64_t {                         // the document that holds byte `pos` (documents tile [0, total))
            int64_t lo = 0, hi = n_docs;
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (offs[mid + 1] <= pos) lo = mid + 1; else hi = mid; }
            return lo;
        };
        // where the matcher may stop reading: the end of the text, or 8 bytes behind the first sync point at or after the block's end
        int64_t cut = -1;
        if (whi == total) cut = total;
        else {
            int64_t f = -1;
            for (int64_t base = b1; base + 8 < whi && f < 0; base += 64) {
                const int64_t i = base + lane;
                const bool ok = i + 8 < whi && tkz_sync_rule(wb(i - 1), wb(i));
                const uint64_t m = simt::ballot(ok);
                if (m) f = base + tkz_ctz64(m);
            }
            const int64_t dn = doc_of(b1);                                  // a document start at or after b1 is a sync point too
            const int64_t ds1 = offs[dn] >= b1 ? offs[dn] : offs[dn + 1];
            if (ds1 + 8 < whi && (f < 0 || ds1 < f)) f = ds1;
            if (f >= 0) cut = f + 8;
        }
        // lane 0 starts from the nearest sync point at or before the block's first byte
        const int64_t d0 = doc_of(b0), a0 = offs[d0];
        int64_t start0 = -1;
        if (a0 == b0) start0 = b0;
        else {
            const int64_t lower = a0 > wlo ? a0 : wlo;                       // candidates i need byte i-1 of the same document inside the window
            for (int64_t base = b0; base > lower && start0 < 0; base -= 64) {
                const int64_t i = base - lane;
                const bool ok = i > lower && tkz_sync_rule(wb(i - 1), wb(i));
                const uint64_t m = simt::ballot(ok);
                if (m) start0 = base - tkz_ctz64(m);
            }
            if (start0 < 0 && a0 >= wlo) start0 = a0;
        }
        if (cut < 0 || start0 < 0) {                                        // no sync point in reach: the block from HBM, one lane
            if (lane == 0) tkz_seq_block_global(bytes, offs, n_docs, total, startbits, pattern, bmp, b0, b1, counters);
            continue;
        }
        // first sync point of every segment, then the first one at or after every segment's start (suffix minimum over the lanes)
        const int64_t t0 = b0 + (int64_t)kSeqSeg * lane, t1 = t0 + kSeqSeg < b1 ? t0 + kSeqSeg : b1;
        int64_t own = b1;
        if (lane > 0 && t0 < b1) {
            for (int64_t i = t0; i < t1; ++i) if (tkz_sync_rule(wb(i - 1), wb(i))) { own = i; break; }
            const int64_t dn = doc_of(t0);
            const int64_t ds1 = offs[dn] >= t0 ? offs[dn] : offs[dn + 1];
            if (ds1 < t1 && ds1 < own) own = ds1;
        }
        int64_t st = own;
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = ((int64_t)simt::shfl((int)(st >> 32), (lane + d) & 63) << 32) | (uint32_t)simt::shfl((int)st, (lane + d) & 63);
            if (lane + d < 64 && o < st) st = o;
        }
        int64_t lim = ((int64_t)simt::shfl((int)(st >> 32), (lane + 1) & 63) << 32) | (uint32_t)simt::shfl((int)st, (lane + 1) & 63);
        if (lane == 63) lim = b1;
        if (lane == 0) st = start0;
        // UTF-8 validation of the chars whose lead byte lies in my segment (lane 0: from the start of the char that holds the block's first byte)
        int bad = 0;
        if (t0 < b1) {
            int64_t v = t0;
            int64_t d = doc_of(v);
            if (lane == 0) { for (int back = 0; v > offs[d] && v > wlo && back < 3 && (wb(v) & 0xC0) == 0x80; ++back) --v; }
            else { for (int k = 0; k < 3 && v < t1 && v > offs[d] && v < offs[d + 1] && (wb(v) & 0xC0) == 0x80; ++k) ++v; }
            while (v < t1) {
                while (offs[d + 1] <= v) ++d;
                const int64_t a = offs[d], e = offs[d + 1];
                TkzDoc doc; doc.b = win + (a - wlo); doc.n = (e < cut ? e : cut) - a; doc.bmp = bmp; doc.by_code_point = pattern == TKZ_PAT_O200K;
                const TkzChar ch = tkz_doc_char(doc, v - a);
                bad |= ch.bad;
                v += ch.len;
            }
        }
        if (simt::ballot(bad != 0)) { if (lane == 0) simt::atomic_or((unsigned*)&counters[0], (unsigned)kErrUtf8); continue; }
        // the matches that start in [st, lim)
        if (st < lim) {
            int64_t pos = st, d = doc_of(st), curw = -1;
            uint64_t acc = 0;
            while (pos < lim) {
                while (offs[d + 1] <= pos) ++d;
                const int64_t a = offs[d], e = offs[d + 1];
                TkzDoc doc; doc.b = win + (a - wlo); doc.n = (e < cut ? e : cut) - a; doc.bmp = bmp; doc.by_code_point = pattern == TKZ_PAT_O200K;
                if (pos >= b0) {
                    if ((pos >> 6) != curw) {
                        if (acc) simt::atomic_or64((unsigned long long*)&startbits[curw], acc);
                        curw = pos >> 6; acc = 0;
                    }
                    acc |= 1ull << (pos & 63);
                }
                pos = a + tkz_match_at(pattern, doc, pos - a);
            }
            if (acc) simt::atomic_or64((unsigned long long*)&startbits[curw], acc);
        }
    }
}

// -------------------------------------------------------------------------------------------------
// k_pretok_seq : one lane per document (any pattern).  startbits must be pre-loaded with docbits.
// -------------------------------------------------------------------------------------------------
TKZ_KERNEL(256) void k_pretok_seq(const uint8_t* bytes, const int64_t* offs, int64_t n_docs, int64_t total, uint64_t* startbits,
                                  int pattern, const uint8_t* bmp, int32_t* counters) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d < n_docs; d += stride) {
        const int64_t a = offs[d], b = offs[d + 1];
        if (b <= a || a < 0 || b > total) continue;       // (bad offsets are reported by k_docmark)
        TkzDoc doc; doc.b = bytes + a; doc.n = b - a; doc.bmp = bmp; doc.by_code_point = pattern == TKZ_PAT_O200K;
        int bad = 0;
        for (int64_t p = 0; p < doc.n;) { const TkzChar c = tkz_doc_char(doc, p); bad |= c.bad; p += c.len; }
        if (bad) { simt::atomic_or((unsigned*)&counters[0], (unsigned)kErrUtf8); continue; }
        int64_t curw = -1; uint64_t acc = 0;
        for (int64_t p = 0; p < doc.n;) {
            const int64_t g = a + p;
            if ((g >> 6) != curw) {
                if (acc) simt::atomic_or64((unsigned long long*)&startbits[curw], acc);
                curw = g >> 6; acc = 0;
            }
            acc |= 1ull << (g & 63);
            p = tkz_match_at(pattern, doc, p);
        }
        if (acc) simt::atomic_or64((unsigned long long*)&startbits[curw], acc);
    }
}

// -------------------------------------------------------------------------------------------------
// The encode stage: PROBE -> MERGE -> PLACE, three kernels joined by one record per piece and a short list of the pieces that missed.
//
// The per-piece driver of the reference (TikTokenizer.cs:250-274) does, for every regex match: whole-piece lookup (:262), else
// BytePairEncode (:268), then appends the ids (:256,264,269).  On the device those three steps have very different shapes --
// 94 % of the pieces of English/code text end at the lookup, a merge is a chain of ~10 dependent table gathers, and the append
// needs a prefix sum over everything before it -- so they are three kernels, each shaped for its own bottleneck, joined by
//
//   prank[p]   one 32-bit record per piece, in piece order.  Sub-tile s owns [pbase[s], pbase[s] + pcount[s]); pbase is the scan of the
//              counts ROUNDED UP TO 16 records, so that every sub-tile's records are whole 64-byte lines of its own: k_probe writes them
//              once, in full lines, k_place reads them once.
//              hit : rank | MARK                          (MARK: a document -- or, at piece granularity, a piece -- starts here)
//              miss: MISS | MARK | idx                    (idx: its entry in the sub-tile's miss list; LONG: the list of the 17+-byte misses)
//                    MISS | GIANT | MARK | relpos         (a piece of more than 1024 bytes: k_giant_*)
//   mlist[s * mcap + i]   the sub-tile's MISS LIST: the misses of <= 16 bytes from the front (i = 0, 1, ...), those of 17..1024 bytes from the
//              back (i = mcap - 1, mcap - 2, ...); mcount[s] = n_short | n_long << 16.  An entry is  relpos | (len - 1) << 10  when k_probe
//              writes it and  DONE | DENSE? | (count - 1) << 12 | offset  once its piece is merged (the merge kernels answer in place).
//              The merge kernels read ONLY these lists (~6 % of the pieces), never the records; mcap starts at 64 entries per sub-tile
//              and the batch is redone once with a larger one when a sub-tile needed more (text where nearly every piece misses).
//   mquad[s * mcap + i]   16 bytes beside every SHORT entry: k_probe leaves the piece's bytes there (it has them in LDS; k_merge_short then needs no
//              gather into the text: ONE coalesced load per entry instead of two scattered requests, twice), and k_merge_short leaves the
//              piece's tokens there when there are at most four (INLINE: k_place gets them in the round trip that fetches the answers).
//   dense[]    the tokens of the merged SHORT pieces of a group of 16 sub-tiles, packed in list order (4096 per group; a miss costs
//              ~4 tokens = one 16-byte store next to its neighbour's, not a 64-byte line of its own in k_merge_short and again in k_place)
//   tmp[b]     4 B per input byte, touched only under LONG missed pieces (and what overflows dense[]): a piece's tokens fit inside
//              its own byte span (tokens <= bytes)
//
//   k_probe        one wavefront per 1 KiB sub-tile, 32 wavefronts per CU: piece enumeration from the bitmap, the 13..28-byte pieces
//                  first (MID table, results parked in LDS), then SHORT probes (the first candidate bucket = two 16-byte gathers per
//                  piece, the second bucket only for the lanes that did not find their key; two batches of 64 pieces in flight; key
//                  dwords computed once and kept), every batch's 64 records stored as four full lines, misses appended to the list
//   k_merge_short  one wavefront per group of 16 sub-tiles: their short-miss lists are packed 64 to a wavefront -- looked up in
//                  the piece memo (the reference's LRUCache on the device), the survivors merged, every lane busy (tkz_bpe_lane) --
//                  instead of the ~14 of 64 a sub-tile has on its own.  Also the per-sub-tile token counts.
//   k_giant_order / k_giant_merge, k_long_* + k_merge_long_q (k_merge_long), k_merge_coop   the rare long ones: > 1024 bytes by a whole workgroup
//                  (tkz_bpe_long_tail: batches of merges that cannot disturb one another, rounds for chains of equal pairs); 17..128 bytes one LANE each in a
//                  span of an LDS arena, 64 pieces of one length class a batch; 129..1024 bytes one WAVEFRONT each, with the workgroup's merger
//   (scan of the token counts)
//   k_place        one wavefront per sub-tile: count per record -> prefix -> ids staged in LDS and stored as whole 16-byte quads at
//                  their final position, token index of every marked piece for the document offsets
// Workgroup b of k_probe / k_merge_short / k_place works on sub-tile range (b % 8) * (n / 8) + b / 8: consecutive sub-tiles -- which share the
// lines at the edges of their id and record ranges -- run on ONE XCD (workgroup b is dispatched to XCD b % 8) and meet in its L2.
// -------------------------------------------------------------------------------------------------
constexpr uint32_t kPrMiss = 1u << 31, kPrMark = 1u << 30, kPrLong = 1u << 29, kPrGiant = 1u << 28;
constexpr uint32_t kPrRankMask = (1u << 28) - 1u;       // ranks are < 2^27 (TKZ_MAX_RANK)
constexpr uint32_t kMrDone = 1u << 31, kMrDense = 1u << 30, kMrInline = 1u << 29;
constexpr int kMrLenShift = 10, kMrCntShift = 12;
constexpr uint32_t kMrOffMask = (1u << kMrCntShift) - 1u;
static_assert(kDenseCap <= (1 << kMrCntShift) && kSub <= (1 << kMrLenShift), "the offset field of a result entry");
#ifndef TKZ_PROBE_U
#define TKZ_PROBE_U 2
#endif
#ifndef TKZ_MS_THREADS
#define TKZ_MS_THREADS 256
#endif
#ifndef TKZ_PROBE_OCC
#define TKZ_PROBE_OCC 8
#endif
constexpr int kGroup = kMergeGroup;                     // sub-tiles per wavefront of k_merge_short
constexpr int kMsThreads = TKZ_MS_THREADS;              // ... and the workgroup size of that kernel
#ifndef TKZ_PROBE_PER
#define TKZ_PROBE_PER 1
#endif
constexpr int kProbePer = TKZ_PROBE_PER;                // consecutive sub-tiles per wavefront of k_probe (the next one's text is requested ahead)
constexpr int kMidMax = kSub / (TKZ_SHORT_KEY_MAX + 1) + 2;   // pieces of 13+ bytes that can start in one sub-tile

// The workgroup a block stands for: blocks b, b + 8, b + 16 ... of a grid run on one XCD (observed dispatch: XCD = b % 8; for speed only,
// nothing depends on it), so XCD x takes the x-th eighth of the work, in order.  nblocks is a multiple of 8.
TKZ_DEV int64_t tkz_xcd_block(int64_t b, int64_t nblocks) { return (b & 7) * (nblocks >> 3) + (b >> 3); }

// exclusive prefix over the wave of a small non-negative value (< 2^BITS), and the wave total;
// bit-sliced: one ballot + mbcnt per bit, no LDS traffic
template <int BITS>
TKZ_DEV int tkz_wave_scan(int v, int* total) {
    const uint64_t below = tkz_lowmask(simt::lane());
    int pre = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < BITS; ++j) {
        const uint64_t m = simt::ballot((v >> j) & 1);
        pre += tkz_popc64(m & below) << j;
        tot += tkz_popc64(m) << j;
    }
    *total = tot;
    return pre;
}

// exclusive prefix sum over the wave of any non-negative value (idle lanes contribute 0: every lane of the wave must be active)
TKZ_DEV int tkz_wave_scan_sum(int v, int* total) {
    const int x = simt::scan_inclusive(v);
    *total = simt::last_lane(x);
    return x - v;
}

// dword i of the key that starts at byte s of the LDS-staged sub-tile, zero-padded past len
TKZ_DEV uint32_t tkz_key_dword(const uint32_t* s_bytes, int s, int len, int i) {
    const int w = (s >> 2) + i;
    const uint32_t x = simt::alignbit(s_bytes[w + 1], s_bytes[w], (uint32_t)(s & 3) * 8u);
    const int nb = len - 4 * i;
    return nb >= 4 ? x : (nb <= 0 ? 0u : (x & ((1u << (8 * nb)) - 1u)));
}

// LDS of one wavefront of the probe stage (+ the mask table, shared by the workgroup)
constexpr int kProbeLdsBytes = (kSub + kHalo) + 2 * (kSub + 2) + 2 * kMidMax + 4 * kMidMax + 4 * (kSub / 32);     // per wavefront; a multiple of 4
constexpr int kProbeLdsQuads = (kProbeLdsBytes + 15) / 16;
struct ProbeLds { uint32_t* bytes; uint16_t* pstart; uint16_t* mid; uint32_t* midres; uint32_t* mark; const uint4* kmask; uint32_t* spec /* k_probe_special only */; };
TKZ_DEV ProbeLds tkz_probe_lds(uint4* wave_quads, const uint4* kmask) {
    ProbeLds L;
    uint8_t* b = reinterpret_cast<uint8_t*>(wave_quads);
    L.bytes = reinterpret_cast<uint32_t*>(b); b += kSub + kHalo;
    L.midres = reinterpret_cast<uint32_t*>(b); b += 4 * kMidMax;
    L.mark = reinterpret_cast<uint32_t*>(b); b += 4 * (kSub / 32);
    L.pstart = reinterpret_cast<uint16_t*>(b); b += 2 * (kSub + 2);
    L.mid = reinterpret_cast<uint16_t*>(b);
    L.kmask = kmask;
    L.spec = nullptr;
    return L;
}
// byte masks of the zero-padded keys, a row per length, written by threads 0..28 of the workgroup and followed by a barrier: rows 0..12 the three dwords of
// a SHORT key; rows 13..28 dwords 3..6 of a MID key, whose first three are always whole (the pre-pass: one LDS read in place of four computed masks)
constexpr int kProbeMaskRows = TKZ_MID_KEY_MAX + 1;
TKZ_DEV void tkz_probe_kmask_init(uint4* s_kmask) {
    if (simt::tid() < kProbeMaskRows) {
        const int len = simt::tid();
        const int first = len <= TKZ_SHORT_KEY_MAX ? 0 : 3;
        uint32_t m[4];
        for (int i = 0; i < 4; ++i) { const int nb = len - 4 * (first + i); m[i] = nb >= 4 ? 0xFFFFFFFFu : (nb <= 0 ? 0u : ((1u << (8 * nb)) - 1u)); }
        uint4 v; v.x = m[0]; v.y = m[1]; v.z = m[2]; v.w = first ? m[3] : 0u;
        s_kmask[len] = v;
    }
}
// the text of a sub-tile (+ halo) in flight: 16 bytes per lane, the halo by lanes 0..3; bytes beyond the corpus read as 0
struct ProbeText { uint4 v0, v1; };
static_assert((kSub + kHalo) / 16 <= 128, "two 16-byte loads per lane cover the sub-tile and its halo");
TKZ_DEV void tkz_probe_request_text(const EncodeParams& P, int64_t sub, ProbeText* tx) {
    const int lane = simt::lane();
    const int64_t base = sub * kSub;
    uint4 v0, v1;
    v0.x = v0.y = v0.z = v0.w = 0; v1 = v0;
    // (a scalar base and 32-bit lane offsets; `left`: the bytes of the sub-tile and its halo that the corpus holds -- wave-uniform)
    const uint8_t* const tb = P.bytes + base;
    const int64_t left64 = P.total - base;
    const int left = left64 >= kSub + kHalo ? kSub + kHalo : (left64 < 0 ? 0 : (int)left64);
    const uint32_t o0 = 16u * (uint32_t)lane, o1 = o0 + 1024u;
    if (left == kSub + kHalo) {                              // an interior sub-tile, nearly every one: no bound a lane
        v0 = tkz_load16_nt(tb + o0);
        if (lane + 64 < (kSub + kHalo) / 16) v1 = tkz_load16_nt(tb + o1);
    } else {                                                 // the corpus ends in here
        if ((int)o0 + 16 <= left) v0 = tkz_load16_nt(tb + o0);
        else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (int j = 0; j < 16; ++j) if ((int)o0 + j < left) w[j >> 2] |= (uint32_t)tb[o0 + (uint32_t)j] << (8 * (j & 3));
            v0.x = w[0]; v0.y = w[1]; v0.z = w[2]; v0.w = w[3];
        }
        if (lane + 64 < (kSub + kHalo) / 16) {
            if ((int)o1 + 16 <= left) v1 = tkz_load16_nt(tb + o1);
            else {
                uint32_t w[4] = {0, 0, 0, 0};
                for (int j = 0; j < 16; ++j) if ((int)o1 + j < left) w[j >> 2] |= (uint32_t)tb[o1 + (uint32_t)j] << (8 * (j & 3));
                v1.x = w[0]; v1.y = w[1]; v1.z = w[2]; v1.w = w[3];
            }
        }
    }
    tx->v0 = v0; tx->v1 = v1;
}
// The special entries: the piece at byte s of the sub-tile, len bytes long, is a TAKEN special-token literal (EncodeParams::specbits) -- its id, from the literal
// table: the first registered literal of that length with those bytes (k_lit_scan took the first registered literal that matches at s: it is this one).
// Rare (a literal per document): the table is read from memory, the bytes from LDS (sb) or, beyond the staged halo, from the text (gb).
// (A UTF-16 special call -- P.lit_repl --: a literal that holds U+FFFD and covers a replaced byte is passed over here as k_lit_scan passed it over; `abs` is the
// piece's byte position in the batch.)
// does [bit, bit + len) of the bitmap rw (nrw words) hold a set bit?  len <= kLitMaxLen: three words at most
TKZ_DEV bool tkz_bits_any(const uint64_t* rw, int64_t nrw, int64_t bit, int len) {
    const int64_t wa = bit >> 6, wb = (bit + len - 1) >> 6;
    for (int64_t w = wa; w <= wb && w < nrw; ++w) {
        uint64_t m = rw[w];
        if (w == wa) m &= ~tkz_lowmask((int)(bit & 63));
        if (w == wb) m &= tkz_lowmask((int)((bit + len - 1) & 63) + 1);
        if (m) return true;
    }
    return false;
}
// literal i of the table holds U+FFFD (meta[kLitFffdHead ..]) and its len bytes at `bit` cover a replaced byte: it does not match there
TKZ_DEV bool tkz_lit_replaced(const uint32_t* meta, int i, const uint64_t* rw, int64_t nrw, int64_t bit, int len) {
    return rw && ((meta[kLitFffdHead + (i >> 5)] >> (i & 31)) & 1u) && tkz_bits_any(rw, nrw, bit, len);
}
TKZ_DEV int32_t tkz_lit_id(const EncodeParams& P, const uint8_t* sb, const uint8_t* gb, int s, int len, int64_t abs) {
    const uint8_t* tx = s + len <= kSub + kHalo ? sb + s : gb + s;
    for (int i = 0; i < P.n_lit; ++i) {
        const uint32_t m = P.lit_meta[kLitMetaHead + 2 * i];
        if ((int)(m >> 16) != len) continue;
        const uint8_t* lit = P.lit_blob + (m & 0xFFFFu);
        int k = 0;
        while (k < len && lit[k] == tx[k]) ++k;
        if (k == len && !tkz_lit_replaced(P.lit_meta, i, P.lit_repl, P.nwords, abs, len)) return (int32_t)P.lit_meta[kLitMetaHead + 2 * i + 1];
    }
    return TKZ_RANK_NONE;
}
// one sub-tile, by one wavefront (no workgroup barrier inside: every wavefront is on its own).  tx: the sub-tile's text, requested by the
// caller; on return it holds the request for sub-tile `next` (< 0: none), issued as soon as this one's text had moved into LDS -- a
// wavefront that probes consecutive sub-tiles never waits for text again.
// REPORT: a list that does not fit is reported here, by two atomics on the counter block (the single-launch kernel: one workgroup); the batch path
// leaves that to k_list_stats, which reads the lengths from mcount -- when nearly every sub-tile overflows (the first batch of text that is
// full of missed pieces) ten million atomics on one line cost 100 ms.
// SPECIAL (k_probe_special, the special entries): a piece whose start is marked in P.specbits is a special-token literal -- its record is the literal's id, it
// takes part in no lookup and is never a miss (not listed, not merged, not in the memo or the miss share).  SPECIAL == false compiles to the code it always was.
template <bool REPORT, bool SPECIAL = false>
TKZ_DEV void tkz_probe_subtile(const TkzTables& T, const EncodeParams& P, int64_t sub, const ProbeLds& LD, ProbeText& tx, int64_t next) {
    const int lane = simt::lane();
    uint32_t* s_bytes = LD.bytes;
    uint16_t* s_pstart = LD.pstart;
    uint16_t* s_mid = LD.mid;
    uint32_t* s_midres = LD.midres;
    uint32_t* s_mark = LD.mark;
    const uint4* s_kmask = LD.kmask;
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(s_bytes);
    const int64_t base = sub * kSub;
    const int nb = (int)(P.total - base < kSub ? P.total - base : kSub);
    const uint8_t* gbase = P.bytes + base;
    const bool prof = TKZ_DEV_FLAG(P, 16);
    long long t_0 = prof ? simt::clock() : 0, t_1 = 0, t_2 = 0, t_3 = 0;
    // ---- everything the wavefront needs from memory is requested first, in ONE round trip: the sub-tile (+ halo), 16 B per lane
    // (the halo by lanes 0..3), the bitmap words one per lane, and the bitmap word after the sub-tile in which the end of its last
    // piece is looked for (the batch kernels: one scalar; k_small: the 64 words after it, one per lane) -- and only then consumed ----
    // (the text itself was requested even earlier: by the caller, or while the sub-tile before this one was probed -- tx)
    uint4 v0 = tx.v0, v1 = tx.v1;
    uint64_t myword = 0, mymark = 0;                      // lanes 0..15: piece-start word / mark word of the sub-tile
    uint64_t myspec = 0;                                  // (SPECIAL: the starts of the taken literals)
    // (every bitmap word at a wave-uniform base plus the lane's 32-bit index, against a 32-bit count of the words that exist: no 64-bit address or
    //  comparison a lane)
    const int64_t wb = sub * (kSub / 64);
    const int64_t wleft64 = P.nwords - wb;
    const int wleft = wleft64 >= kSub / 64 ? kSub / 64 : (wleft64 < 0 ? 0 : (int)wleft64);      // the sub-tile's words that exist: all 16, but for the last sub-tile
    if (lane < wleft) {
        const uint32_t wl = (uint32_t)lane;
        myword = (P.startbits + wb)[wl]; mymark = (P.docbits + wb)[wl]; if (SPECIAL) myspec = (P.specbits + wb)[wl];
    }
    const int64_t from = base + nb, w0 = from >> 6;        // the search for the end of the last piece starts here
    const int64_t aleft64 = P.nwords - w0;
    const int aleft = aleft64 >= 64 ? 64 : (aleft64 < 0 ? 0 : (int)aleft64);                    // of the 64 words from w0 on, those that exist
    // The batch kernels: the first of those words is at a wave-uniform address and nearly always holds a piece start (a piece is a few bytes long), so it is
    // read as a scalar and searched on the scalar side; the 64 lanes' words are only asked for when it holds none.  k_small wrote the bitmap in this very
    // launch -- a scalar cache may hold what was there before --: it keeps the lanes' loads.
    int64_t last_end = -1;
    uint64_t ahead = 0;
    if constexpr (REPORT) { if (lane < aleft) ahead = (P.startbits + w0)[(uint32_t)lane]; }
    else if (aleft > 0) {
        const uint64_t v = simt::uniform64(P.startbits[w0]) & ~tkz_lowmask((int)(from & 63));
        if (v) last_end = (w0 << 6) + tkz_ctz64(v);
    }
    const int64_t pb = (int64_t)simt::uniform64((uint64_t)P.pbase[sub]);
    // ---- consume ----
    { uint4* s4 = reinterpret_cast<uint4*>(s_bytes); s4[lane] = v0; if (lane + 64 < (kSub + kHalo) / 16) s4[lane + 64] = v1; }
    if (next >= 0) tkz_probe_request_text(P, next, &tx);
    if (lane < kSub / 64) {
        const int lim = nb - lane * 64;                    // bits at or beyond the end of the corpus are not pieces
        if (lim <= 0) myword = 0; else if (lim < 64) myword &= tkz_lowmask(lim);
        s_mark[2 * lane] = (uint32_t)mymark; s_mark[2 * lane + 1] = (uint32_t)(mymark >> 32);
        if (SPECIAL) { LD.spec[2 * lane] = (uint32_t)myspec; LD.spec[2 * lane + 1] = (uint32_t)(myspec >> 32); }
    }
    // end of the last piece that starts here = first piece start at or after base+nb (the sentinel at `total` bounds it)
    if (last_end < 0) {
        int64_t found = -1;
        for (int64_t c = 0; found < 0; ++c) {
            const int64_t w = w0 + c * 64 + lane;
            uint64_t v = (REPORT && c == 0) ? ahead : (w < P.nwords ? P.startbits[w] : 0);
            if (w == w0) v &= ~tkz_lowmask((int)(from & 63));
            const uint64_t any = simt::ballot(v != 0);
            if (any) {
                const int src = tkz_ctz64(any);
                const uint32_t lo = simt::shflu((uint32_t)v, src), hi = simt::shflu((uint32_t)(v >> 32), src);
                found = ((w0 + c * 64 + src) << 6) + tkz_ctz64(((uint64_t)hi << 32) | lo);
            } else if (w0 + (c + 1) * 64 >= P.nwords) found = P.total;
        }
        last_end = found;
    }
    // (anything beyond kArenaPiece bytes is a giant piece, whose real length k_giant_find takes from the bitmap)
    const int last_end_rel = (int)(last_end - base < 2 * kSub + 2 ? last_end - base : 2 * kSub + 2);
    // ---- ordered compaction of the piece starts (bit-sliced ballot prefix, no LDS scan) ----
    const uint32_t wlo = simt::shflu((uint32_t)myword, lane >> 2), whi = simt::shflu((uint32_t)(myword >> 32), lane >> 2);
    const uint32_t bits16 = (uint32_t)(((((uint64_t)whi << 32) | wlo) >> (16 * (lane & 3))) & 0xFFFFull);
    int np;
    {
        int off = tkz_wave_scan<5>(tkz_popc32(bits16), &np);
        for (uint32_t b = bits16; b; b &= b - 1) s_pstart[off++] = (uint16_t)(16 * lane + tkz_ctz32(b));
        if (lane == 0) s_pstart[np] = (uint16_t)last_end_rel;         // (sentinel: the length of piece k is s_pstart[k + 1] - s_pstart[k])
    }
    (void)simt::ballot(true);                              // (LDS written by other lanes of this wavefront is read below)
    // nrec: the sub-tile's records that the buffer holds -- all np of them, unless the attempt is one to be thrown away.  What the wavefront has to say that
    // does not depend on the lookups is said here, so that no pointer or bound it takes is held in scalar registers across the loops: the token count zeroed
    // for the merge kernels of both streams, which add to it (launch_encode), and a record buffer that is too small.
    const int64_t room64 = P.prank_cap - pb;
    const int nrec = room64 < np ? (room64 < 0 ? 0 : (int)room64) : np;
    if (lane == 0) {
        if (!REPORT && P.tc_atomic) P.tile_count[sub] = 0;
        if (room64 < np) simt::atomic_or((unsigned*)&P.counters[0], (unsigned)kErrCapacity);
    }
    if (prof) t_1 = simt::clock();
    const char* tb0 = reinterpret_cast<const char*>(T.short_slots);
    const uint32_t mid_off = (uint32_t)(reinterpret_cast<const char*>(T.mid_slots) - tb0);   // (SHORT and MID share one allocation)
    // ---- the pieces of 13+ bytes first: a few per cent of all pieces, twice the instructions of a short one (13..28 bytes: MID table;
    // 29..1024: the LONG table, rare).  Looked up together, 64 per batch, and their answers parked in LDS by ordinal: the main loop below
    // then handles nothing but keys of up to 12 bytes and stores every batch's 64 records as four FULL lines (patching these few records
    // in afterwards punched holes into every line: 1.7x the write traffic) ----
    int nmid = 0;
#pragma unroll 1
    for (int k0 = 0; k0 < np; k0 += 64) {
        const int k = k0 + lane;
        int len = 0;
        if (k < np) len = (int)s_pstart[k + 1] - (int)s_pstart[k];
        const uint64_t midm = simt::ballot(len > TKZ_SHORT_KEY_MAX && len <= kArenaPiece);
        if ((midm >> lane) & 1ull) s_mid[nmid + tkz_popc64(midm & tkz_lowmask(lane))] = (uint16_t)k;
        nmid += tkz_popc64(midm);
    }
    (void)simt::ballot(true);
#pragma unroll 1
    for (int m0 = 0; m0 < nmid; m0 += 64) {
        const bool valid = m0 + lane < nmid;
        int s = 0, len = 13;
        uint32_t kk[7] = {0, 0, 0, 0, 0, 0, 0}, oa = 0, ob = 0;
        if (valid) {
            const int k = s_mid[m0 + lane];
            s = s_pstart[k];
            len = (int)s_pstart[k + 1] - s;
        }
        const bool is_lit = SPECIAL && valid && ((LD.spec[s >> 5] >> (s & 31)) & 1u);
        const bool is_mid = valid && len <= TKZ_MID_KEY_MAX && !is_lit;
        if (is_mid) {
            // the key's seven dwords, zero-padded: eight aligned dwords read once, seven v_alignbit, and the masks of dwords 3..6 from the row of the
            // key's length (13..28 here: the first three dwords are whole; the eighth dword ends at byte 1051 of the staged 1088 at the latest)
            const int w = s >> 2;
            const uint32_t sh = (uint32_t)(s & 3) * 8u;
            uint32_t d[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = s_bytes[w + i];
#pragma unroll
            for (int i = 0; i < 7; ++i) kk[i] = simt::alignbit(d[i + 1], d[i], sh);
            const uint4 km = s_kmask[len];
            kk[3] &= km.x; kk[4] &= km.y; kk[5] &= km.z; kk[6] &= km.w;
            uint32_t s1, s2;
            tkz_mid_slots(T, kk, (uint32_t)len, &s1, &s2);
            oa = mid_off + 32u * s1; ob = mid_off + 32u * s2;
        }
        const uint4 a0 = tkz_load16(tb0 + oa), a1 = tkz_load16(tb0 + oa + 16u), b0 = tkz_load16(tb0 + ob), b1 = tkz_load16(tb0 + ob + 16u);
        int32_t rank = TKZ_RANK_NONE;
        if (is_mid) rank = tkz_match_mid(kk, (uint32_t)len, a0, a1, b0, b1);
        else if (is_lit) rank = tkz_lit_id(P, sb, gbase, s, len, base + s);
        else if (valid) {
            if (s + len <= kSub + kHalo) rank = tkz_lookup_long(T, [&](int i) -> uint32_t { return sb[s + i]; }, (uint32_t)len);
            else rank = tkz_lookup_long(T, [&](int i) -> uint32_t { return gbase[s + i]; }, (uint32_t)len);
        }
        if (valid) s_midres[m0 + lane] = (uint32_t)rank;
    }
    (void)simt::ballot(true);
    if (prof) t_2 = simt::clock();
    // ---- the main loop: two batches of 64 pieces per iteration, their gathers in flight together (what a sub-tile costs is its count of
    // dependent round trips to the tables) ----
    // (the lists and the records: wave-uniform bases and a lane's 32-bit byte offset -- a list has at most kMissCapMax entries)
    uint32_t* const ml = P.mlist + sub * (int64_t)P.mcap;
    uint4* const mq = P.mquad + sub * (int64_t)P.mcap;
    auto ml_at = [&](int i) -> uint32_t* { return reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ml) + 4u * (uint32_t)i); };
    auto mq_at = [&](int i) -> uint4* { return reinterpret_cast<uint4*>(reinterpret_cast<char*>(mq) + 16u * (uint32_t)i); };
    int32_t* const recs = P.prank + pb;
    const int mcap = P.mcap, lane_piece = P.lane_piece;
    const bool has_pextra = P.pextra != nullptr;          // (wave-uniform: only when the tables hold promoted pieces)
    int ns = 0, nl = 0, midseen = 0;
    int promo_extra = 0;                                   // tokens beyond one per piece that the promoted pieces of this sub-tile stand for (P.pextra): this lane's share
    bool giant = false, coopl = false;                     // coopl: a long miss of more than kLanePiece bytes (k_merge_coop's: bit 2 of the sub-tile's flag)
    constexpr int U = TKZ_PROBE_U;                         // batches of 64 pieces whose gathers are in flight together
#ifdef TKZ_DEVPROF
    // (development counters: where the main loop's ticks go and how many lanes each part has switched on -- the lane-cycle table of DESIGN.md 3)
    long long pf_first = 0, pf_second = 0, pf_emit = 0, pf_t = 0;
    int pf_batches = 0, pf_valid = 0, pf_want2 = 0, pf_iters2 = 0;
#define TKZ_PROBE_MARK(acc) do { if (prof) { const long long pf_now = simt::clock(); acc += pf_now - pf_t; pf_t = pf_now; } } while (0)
    if (prof) pf_t = simt::clock();
#else
#define TKZ_PROBE_MARK(acc) do { } while (0)
#endif
#pragma unroll 1
    for (int k0 = 0; k0 < np; k0 += 64 * U) {
        int ps[U], plen[U];
        uint32_t hs[U], kw0[U], kw1[U], kw2[U];
        uint4 a0[U], a1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + 64 * u + lane;
            ps[u] = 0; plen[u] = 0;
            if (k < np) { ps[u] = s_pstart[k]; plen[u] = (int)s_pstart[k + 1] - ps[u]; }
            // the key's three dwords, zero-padded: four aligned dwords, three v_alignbit, one mask row -- computed ONCE and kept
            const int s = ps[u], w = s >> 2;
            const uint32_t sh = (uint32_t)(s & 3) * 8u;
            const uint32_t d0 = s_bytes[w], d1 = s_bytes[w + 1], d2 = s_bytes[w + 2], d3 = s_bytes[w + 3];
            const bool is_short = plen[u] >= 1 && plen[u] <= TKZ_SHORT_KEY_MAX;
            const uint4 km = s_kmask[is_short ? plen[u] : 0];
            kw0[u] = simt::alignbit(d1, d0, sh) & km.x; kw1[u] = simt::alignbit(d2, d1, sh) & km.y; kw2[u] = simt::alignbit(d3, d2, sh) & km.z;
            const uint32_t slot = tkz_short_slot_first(T, kw0[u], kw1[u], kw2[u], (uint32_t)plen[u], &hs[u]);
            // the FIRST candidate bucket of every piece (idle lanes and longer pieces gather slot 0: a load inside a divergent branch
            // is waited for inside it)
            const uint32_t oa = simt::lane_offset(is_short ? 16u * slot : 0u);
            a0[u] = tkz_load16(tb0 + oa); a1[u] = tkz_load16(tb0 + oa + 16u);
        }
        int32_t rk[U];
        bool more = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool is_short = plen[u] >= 1 && plen[u] <= TKZ_SHORT_KEY_MAX;
            rk[u] = tkz_match_short2x(kw0[u], kw1[u], kw2[u], (uint32_t)plen[u], a0[u], a1[u]);       // (a piece that is not short matches no slot: len 0 or > 12)
            if (SPECIAL && is_short && ((LD.spec[ps[u] >> 5] >> (ps[u] & 31)) & 1u)) rk[u] = tkz_lit_id(P, sb, gbase, ps[u], plen[u], base + ps[u]);
            more = more || (is_short && rk[u] == TKZ_RANK_NONE);
        }
        // the second bucket, for the lanes the first one did not settle only (the keys the builder could not keep in their first
        // bucket, and the pieces that are not keys at all): ~15 % of the requests of the first step instead of another 100 %
        bool two_pass = simt::ballot(more) != 0;
        TKZ_PROBE_MARK(pf_first);
#ifdef TKZ_DEVPROF
        if (prof) {
            for (int u = 0; u < U; ++u) { const int nv = np - (k0 + 64 * u); if (nv > 0) { ++pf_batches; pf_valid += nv < 64 ? nv : 64; } }
            for (int u = 0; u < U; ++u) pf_want2 += tkz_popc64(simt::ballot(plen[u] >= 1 && plen[u] <= TKZ_SHORT_KEY_MAX && rk[u] == TKZ_RANK_NONE));
            pf_iters2 += two_pass ? 1 : 0;
            pf_t = simt::clock();
        }
#endif
        if (two_pass) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool want = plen[u] >= 1 && plen[u] <= TKZ_SHORT_KEY_MAX && rk[u] == TKZ_RANK_NONE;
                if (want) {
                    const uint32_t ob = simt::lane_offset(16u * tkz_short_slot_second(T, hs[u]));
                    a0[u] = tkz_load16(tb0 + ob); a1[u] = tkz_load16(tb0 + ob + 16u);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool want = plen[u] >= 1 && plen[u] <= TKZ_SHORT_KEY_MAX && rk[u] == TKZ_RANK_NONE;
                if (want) rk[u] = tkz_match_short2x(kw0[u], kw1[u], kw2[u], (uint32_t)plen[u], a0[u], a1[u]);
            }
        }
        TKZ_PROBE_MARK(pf_second);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + 64 * u + lane;
            const bool valid = k < np;
            const int s = ps[u], len = plen[u];
            const bool is_mid = len > TKZ_SHORT_KEY_MAX && len <= kArenaPiece;
            const uint64_t midm = simt::ballot(is_mid);
            int32_t rank = rk[u];                                                // Encoder.TryGetValue(piece) (TikTokenizer.cs:262)
            if (is_mid) rank = (int32_t)s_midres[midseen + tkz_popc64(midm & tkz_lowmask(lane))];
            midseen += tkz_popc64(midm);
            const bool is_giant = len > kArenaPiece;                             // (k_giant_merge looks a giant piece up itself)
            const bool miss = valid && !is_giant && rank == TKZ_RANK_NONE;
            if (has_pextra) {
                const uint32_t ex = (valid && !is_giant && !miss && ((uint32_t)rank & kPromoFlag)) ? (((uint32_t)rank >> kPromoCntShift) & 3u) : 0u;
                promo_extra += (int)ex;                                          // (per lane: one add a batch; summed over the wavefront once, at the end)
            }
            const bool miss_s = miss && len <= kShortMax, miss_l = miss && len > kShortMax;
            const uint64_t sm = simt::ballot(miss_s), lm = simt::ballot(miss_l);
            const int is_ = ns + tkz_popc64(sm & tkz_lowmask(lane)), il = nl + tkz_popc64(lm & tkz_lowmask(lane));
            ns += tkz_popc64(sm); nl += tkz_popc64(lm);
            // (the two lists grow towards each other; an entry that would run into the other list is not written -- ns + nl > mcap is then
            //  reported below and the batch redone with longer lists)
            const uint32_t ent = (uint32_t)s | ((uint32_t)(len - 1) << kMrLenShift);
            if (miss_s && is_ + nl < mcap) {
                *ml_at(is_) = ent;
                uint4 kq; kq.x = kw0[u]; kq.y = kw1[u]; kq.z = kw2[u]; kq.w = 0;          // the piece's bytes, zero-padded, for k_merge_short
                if (len > TKZ_SHORT_KEY_MAX) { kq.x = tkz_key_dword(s_bytes, s, len, 0); kq.y = tkz_key_dword(s_bytes, s, len, 1); kq.z = tkz_key_dword(s_bytes, s, len, 2); kq.w = tkz_key_dword(s_bytes, s, len, 3); }
                *mq_at(is_) = kq;
            }
            if (miss_l && il + ns < mcap) *ml_at(mcap - 1 - il) = ent;
            uint32_t rec = ((s_mark[s >> 5] >> (s & 31)) & 1u) ? kPrMark : 0u;
            if (REPORT) giant = giant || (miss_l && len > kSmallLanePiece);      // (k_small, the only REPORT user, hands a batch with such a piece back like one with a giant piece: k_merge_coop is a kernel of the batch path)
            else coopl = coopl || (miss_l && len > lane_piece);
            if (is_giant) { rec |= kPrMiss | kPrGiant | (uint32_t)s; giant = giant || valid; }
            else if (miss) rec |= kPrMiss | (miss_l ? (kPrLong | (uint32_t)il) : (uint32_t)is_);
            else rec |= (uint32_t)rank;
            if (k < nrec) tkz_store_nt(&recs[(uint32_t)k], (int32_t)rec);
        }
        TKZ_PROBE_MARK(pf_emit);
    }
#undef TKZ_PROBE_MARK
#ifdef TKZ_DEVPROF
    if (prof && lane == 0) {
        simt::atomic_add64(&P.devprof[48], (unsigned long long)pf_first); simt::atomic_add64(&P.devprof[49], (unsigned long long)pf_second);
        simt::atomic_add64(&P.devprof[50], (unsigned long long)pf_emit); simt::atomic_add64(&P.devprof[51], (unsigned long long)pf_batches);
        simt::atomic_add64(&P.devprof[52], (unsigned long long)pf_valid); simt::atomic_add64(&P.devprof[53], (unsigned long long)pf_want2);
        simt::atomic_add64(&P.devprof[54], (unsigned long long)pf_iters2);
    }
#endif
    if (prof && lane == 0) {
        t_3 = simt::clock();
        simt::atomic_add64(&P.devprof[0], 1); simt::atomic_add64(&P.devprof[1], (unsigned long long)(t_3 - t_0));
        simt::atomic_add64(&P.devprof[2], (unsigned long long)(t_1 - t_0)); simt::atomic_add64(&P.devprof[3], (unsigned long long)(t_3 - t_2));
        simt::atomic_add64(&P.devprof[4], (unsigned long long)(t_2 - t_1)); simt::atomic_add64(&P.devprof[5], (unsigned long long)nmid);
        simt::atomic_add64(&P.devprof[6], (unsigned long long)np);
    }
    // sub-tiles with long misses (bit 0: statistics only, the lists say it), a giant piece (bit 1: k_giant_find, k_merge_long, k_place), a long miss of more
    // than kLanePiece bytes (bit 2: k_merge_coop -- k_merge_long used to flag those chunks itself: a pointer, an index and a flag alive across its merge
    // loops, 14 more spilled scalars and 4 % of that kernel on mixed text)
    const uint32_t f = (nl ? 1u : 0u) | (simt::ballot(giant) ? 2u : 0u) | (simt::ballot(coopl) ? 4u : 0u);
    if (has_pextra) { int tot; (void)tkz_wave_scan_sum(promo_extra, &tot); promo_extra = tot; }      // (wave-uniform branch)
    if (lane == 0) {
        P.heavy_flag[sub] = (uint8_t)f;
        P.mcount[sub] = (uint32_t)ns | ((uint32_t)nl << 16);
        if (has_pextra) P.pextra[sub] = promo_extra;
        if (REPORT && ns + nl > mcap) { simt::atomic_or((unsigned*)&P.counters[0], (unsigned)kErrMissCap); simt::atomic_max((unsigned*)&P.counters[1], (unsigned)(ns + nl)); }
    }
}
TKZ_KERNEL_OCC(256, TKZ_PROBE_OCC) void k_probe(TkzTables T, EncodeParams P) {
    TKZ_SHARED uint4 s_wave[kThreads / 64][kProbeLdsQuads];
    TKZ_SHARED uint4 s_kmask[kProbeMaskRows];
    tkz_probe_kmask_init(s_kmask);
    simt::sync();                                         // (the only workgroup barrier: from here on every wavefront is on its own)
    const int64_t sub0 = (tkz_xcd_block(simt::bid(), simt::nblocks()) * (kThreads / 64) + simt::wave()) * kProbePer;
    if (sub0 >= P.nsub) return;
    const ProbeLds LD = tkz_probe_lds(s_wave[simt::wave()], s_kmask);
    ProbeText tx;
    tkz_probe_request_text(P, sub0, &tx);
#pragma unroll 1
    for (int it = 0; it < kProbePer && sub0 + it < P.nsub; ++it) {
        const int64_t nxt = (it + 1 < kProbePer && sub0 + it + 1 < P.nsub) ? sub0 + it + 1 : -1;
        tkz_probe_subtile<false>(T, P, sub0 + it, LD, tx, nxt);
        (void)simt::ballot(true);                             // (the next sub-tile reuses the wavefront's LDS)
    }
}

// the special entries' form: the same sub-tiles, with the starts of the taken literals beside the marks
TKZ_KERNEL_OCC(256, TKZ_PROBE_OCC) void k_probe_special(TkzTables T, EncodeParams P) {
    TKZ_SHARED uint4 s_wave[kThreads / 64][kProbeLdsQuads];
    TKZ_SHARED uint4 s_kmask[kProbeMaskRows];
    TKZ_SHARED uint32_t s_spec[kThreads / 64][kSub / 32];
    tkz_probe_kmask_init(s_kmask);
    simt::sync();
    const int64_t sub0 = (tkz_xcd_block(simt::bid(), simt::nblocks()) * (kThreads / 64) + simt::wave()) * kProbePer;
    if (sub0 >= P.nsub) return;
    ProbeLds LD = tkz_probe_lds(s_wave[simt::wave()], s_kmask);
    LD.spec = s_spec[simt::wave()];
    ProbeText tx;
    tkz_probe_request_text(P, sub0, &tx);
#pragma unroll 1
    for (int it = 0; it < kProbePer && sub0 + it < P.nsub; ++it) {
        const int64_t nxt = (it + 1 < kProbePer && sub0 + it + 1 < P.nsub) ? sub0 + it + 1 : -1;
        tkz_probe_subtile<false, true>(T, P, sub0 + it, LD, tx, nxt);
        (void)simt::ballot(true);
    }
}

// the 16 bytes of the corpus that start at byte position `abs`, as four little-endian dwords: the five dwords around them are fetched
// with TWO requests per lane (16 + 4 bytes from the dword-aligned address; a scattered gather costs a request per lane and instruction)
struct alignas(4) TkzDwords4 { uint32_t x, y, z, w; };
TKZ_DEV void tkz_load_piece16(const uint8_t* bytes, int64_t total, int64_t abs, uint32_t* pw) {
    const int64_t a0 = abs & ~(int64_t)3;
    const uint32_t sh = (uint32_t)(abs & 3) * 8u;
    uint32_t w[5];
    if (a0 + 20 <= total) {
        const TkzDwords4 v = *reinterpret_cast<const TkzDwords4*>(bytes + a0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        w[4] = *reinterpret_cast<const uint32_t*>(bytes + a0 + 16);
    } else {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int64_t p = a0 + 4 * i;
            if (p + 4 <= total) w[i] = *reinterpret_cast<const uint32_t*>(bytes + p);
            else { w[i] = 0; for (int j = 0; j < 4; ++j) if (p + j < total) w[i] |= (uint32_t)bytes[p + j] << (8 * j); }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) pw[i] = simt::alignbit(w[i + 1], w[i], sh);
}

// the result a merge kernel leaves in a miss-list entry: the piece's tokens wait in dense[group * kDenseCap + off ..) (DENSE) or in tmp at
// the piece's own byte position (off = relpos)
TKZ_HD uint32_t tkz_result_entry(bool dense, int cnt, int off) { return kMrDone | (dense ? kMrDense : 0u) | ((uint32_t)(cnt - 1) << kMrCntShift) | (uint32_t)off; }
TKZ_HD uint32_t tkz_result_inline(int cnt) { return kMrDone | kMrInline | ((uint32_t)(cnt - 1) << kMrCntShift); }       // <= 4 tokens, in the entry's quad
TKZ_HD int tkz_result_cnt(uint32_t r) { return (int)((r >> kMrCntShift) & 1023u) + 1; }
TKZ_HD int tkz_result_off(uint32_t r) { return (int)(r & kMrOffMask); }

// largest q in [0, N) with pre[q] <= g  (pre: non-decreasing exclusive prefix sums in LDS, g below the total): the list a position belongs to
template <int N, class Pre>
TKZ_DEV int tkz_find_list(const Pre* pre, int g) {
    int q = 0;
#pragma unroll
    for (int step = N / 2; step >= 1; step >>= 1) if (pre[q + step] <= g) q += step;
    return q;
}

// k_merge_short: one wavefront per group of kGroup = 16 sub-tiles.  It walks the group's short-miss lists (k_probe's mlist: ~14 entries per
// sub-tile) 64 entries at a time; the entries that have not been looked up yet go through the PIECE MEMO (the device form of the
// reference's LRUCache, tkz_tables.h): a hit has its <= 4 tokens at once, the survivors stay in the wave's list, and only when that is
// full of survivors are 64 of them merged, one per lane (BytePairEncode, TikTokenizer.cs:268).  Merged pieces of <= 4 tokens claim
// their memo slot if it is empty.  On the bench corpus 3 of 4 missed pieces are memo hits: a merge costs ~45 scattered gathers and ~8
// dependent round trips, a memo lookup 4 and one.  Every entry is answered in place (tkz_result_entry); the records are never read.
// (LDS: 4 x 9.25 KB of merge state + 2.3 KB = 40 KB per workgroup, and <= 128 VGPRs: four workgroups = 16 wavefronts per CU)
constexpr int kMsStride = TkzBpeGeom<16>::kStride, kMsIdStride = TkzBpeGeom<16>::kIdStride;
#ifndef TKZ_MS_SHORT_LEN
#define TKZ_MS_SHORT_LEN 8
#endif
#ifndef TKZ_MS_TWO_MIN
#define TKZ_MS_TWO_MIN 320
#endif
constexpr int kMsTwoListsMin = TKZ_MS_TWO_MIN;         // ... when the group's lists hold at least this many entries
constexpr int kMsShortLen = TKZ_MS_SHORT_LEN;          // k_merge_short's two lists: pieces of up to this many bytes | longer ones
// LDS of one wavefront of k_merge_short (+ the byte-id table shared by the workgroup)
struct MsLds { uint4* pr; uint32_t* ids; uint16_t* rec; uint16_t* idx; int* extra; uint16_t* pre; const uint16_t* brank16; };
// (four workgroups of four wavefronts a CU: 40,960 bytes a workgroup with the 512 of the byte-id table -- 10,112 a wavefront at most)
constexpr int kMsLdsBytes = kMsStride * 64 * 4 + kMsIdStride * 64 * 4 + 2 * (2 * 64 + 2 * 64) + 4 * kGroup + 2 * (kGroup + 1);   // per wavefront, rounded to 16 below
constexpr int kMsLdsQuads = (kMsLdsBytes + 15) / 16;
static_assert((kMsThreads / 64) * kMsLdsQuads * 16 + 512 <= 40960, "k_merge_short: four workgroups a CU (160 KB of LDS, allocated in units of 1,280 bytes)");
TKZ_DEV MsLds tkz_ms_lds(uint4* wave_quads, const uint16_t* brank16) {
    MsLds L;
    uint8_t* b = reinterpret_cast<uint8_t*>(wave_quads);
    L.pr = reinterpret_cast<uint4*>(b); b += kMsStride * 64 * 4;              // per lane pr[16] at a conflict-free stride for 16-byte reads
    L.ids = reinterpret_cast<uint32_t*>(b); b += kMsIdStride * 64 * 4;        // per lane ids[16]
    L.extra = reinterpret_cast<int*>(b); b += 4 * kGroup;                     // tokens the merges added to every sub-tile of the group
    // the wave's TWO lists of pieces that missed the memo (up to 8 bytes | 9..16 bytes), 64 entries each: relpos | (len-1) << 10, and
    // (sub-tile of the group) << 10 | index in its miss list
    L.rec = reinterpret_cast<uint16_t*>(b); b += 2 * 2 * 64;
    L.idx = reinterpret_cast<uint16_t*>(b); b += 2 * 2 * 64;
    L.pre = reinterpret_cast<uint16_t*>(b);                                   // exclusive prefix of the lists' lengths (16 lists of at most 1,024 entries)
    L.brank16 = brank16;
    return L;
}
// the id of every single byte in LDS, not 16 gathers per piece (0xFFFF: not a key, 0xFFFE: too large for 16 bits, look it up); by the whole
// workgroup, followed by a barrier
TKZ_DEV void tkz_ms_brank_init(const TkzTables& T, uint16_t* s_brank16) {
    for (int i = simt::tid(); i < 256; i += simt::nthreads()) {
        const uint32_t v = (uint32_t)T.byte_rank[i];
        s_brank16[i] = (uint16_t)(v >= (uint32_t)TKZ_PSEUDO_BASE ? 0xFFFFu : (v < 0xFFFEu ? v : 0xFFFEu));
    }
}
// one group of kGroup sub-tiles, by one wavefront
TKZ_DEV void tkz_merge_short_group(const TkzTables& T, const EncodeParams& P, int64_t grp, const MsLds& LD) {
    constexpr int NMAX = 16, STRIDE = kMsStride, IDSTRIDE = kMsIdStride;
    static_assert(kGroup == 16 && kShortMax == 16, "list entries: 4 bits of sub-tile, 10 of index; 10 of relpos, 4 of length, 1 flag");
    const int lane = simt::lane();
    const uint16_t* s_brank16 = LD.brank16;
    auto byte_id = [&](uint32_t b) -> uint32_t {
        const uint32_t v = s_brank16[b];
        return v < 0xFFFEu ? v : (v == 0xFFFFu ? (uint32_t)TKZ_PSEUDO_BASE + b : (uint32_t)T.byte_rank[b]);
    };
    auto pair_rank = [&](uint32_t b0, uint32_t b1) -> int32_t { return T.bytepair_rank[(b0 << 8) | b1]; };
    const int64_t sub0 = grp * kGroup;
    if (sub0 >= P.nsub) return;
    uint16_t* s_rec = LD.rec;
    uint16_t* s_idx = LD.idx;
    int* s_extra = LD.extra;
    uint16_t* s_pre = LD.pre;
    uint32_t* ids = LD.ids + lane * IDSTRIDE;
    uint32_t* pr = reinterpret_cast<uint32_t*>(LD.pr) + lane * STRIDE;
    // lane q < kGroup looks after sub-tile q of the group: how many pieces start there, how long its short-miss list is
    int my_np = 0, my_ns = 0;
    if (lane < kGroup && sub0 + lane < P.nsub) { my_np = P.pcount[sub0 + lane]; my_ns = (int)(P.mcount[sub0 + lane] & 0xFFFFu); }
    // (a list longer than mcap was cut by k_probe, which has reported it: the batch is redone; keep to what was written)
    { const int nl_ = lane < kGroup && sub0 + lane < P.nsub ? (int)(P.mcount[sub0 + lane] >> 16) : 0; if (my_ns + nl_ > P.mcap) my_ns = 0; }
    int ntotal;
    { const int pre = tkz_wave_scan_sum(my_ns, &ntotal); if (lane <= kGroup) s_pre[lane] = (uint16_t)pre; }
    if (lane < kGroup) s_extra[lane] = 0;
    uint32_t* const ml0 = P.mlist + sub0 * (int64_t)P.mcap;
    int err = 0, dused = 0, done = 0;
    int nl0 = 0, nl1 = 0;                                       // entries in the wave's two lists (pieces of up to kMsShortLen bytes | longer ones): all have missed the memo
    int st_look = 0, st_hit = 0;                                // TKZ_OPT_PIECE_STATS: memo lookups and hits of this group (one pair of atomics at its end)
    int32_t* const dense = P.dense + grp * kDenseCap;
    const bool memo = T.memo_n != 0;
    // a LEARNING batch (tkz_api.cpp, promote_from_memo): hits of every eighth group are sampled per memo slot (memo_phase below) -- the host promotes
    // the hottest entries into the SHORT / MID tables afterwards.  Null in every other batch.
    const bool sparse = T.memo_hits_sparse != 0;                            // (a large batch: every eighth group, one lane a time; a small one: every hit)
    const bool count_hits = T.memo_hits != nullptr && (!sparse || (grp & 7) == 0);       // (wave-uniform)
    // where the `cnt` tokens of a piece go -- up to four: into the entry's own quad (the caller stores them); more: packed behind those of
    // the pieces before it in the group's dense region (in tmp, at the piece's own byte position, once that is full) -- and the answer in
    // its list entry; every lane of the wavefront calls it (a scan inside)
    auto assign = [&](bool have, int cnt, int si, int j, int rel) -> int32_t* {
        int btot;
        const bool big = have && cnt > 4;
        const int doff = dused + tkz_wave_scan_sum(big ? cnt : 0, &btot);
        int32_t* dst = nullptr;
        if (have) {
            if (!big) ml0[si * (int64_t)P.mcap + j] = tkz_result_inline(cnt);
            else {
                const bool packed = doff + cnt <= kDenseCap;
                dst = packed ? dense + doff : P.tmp + ((sub0 + si) * kSub + rel);
                ml0[si * (int64_t)P.mcap + j] = tkz_result_entry(packed, cnt, packed ? doff : rel);
            }
            if (cnt > 1) simt::atomic_add(&s_extra[si], cnt - 1);
        }
        dused += btot;
        return dst;
    };
    // the piece of a list entry: its 16 bytes, zero beyond its length, as k_probe left them beside the entry; *nul = it holds a zero byte
    uint4* const mq0 = P.mquad + sub0 * (int64_t)P.mcap;
    auto key_of = [&](uint4 kq, int len, uint32_t* kw, bool* nul) {
        kw[0] = kq.x; kw[1] = kq.y; kw[2] = kq.z; kw[3] = kq.w;
        uint32_t z = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int nb = len - 4 * i;
            const uint32_t m = nb >= 4 ? 0xFFFFFFFFu : (nb <= 0 ? 0u : ((1u << (8 * nb)) - 1u));
            z |= (kw[i] - 0x01010101u) & ~kw[i] & 0x80808080u & m;
        }
        *nul = z != 0;
    };
    // the entries that have not been through the memo: hits are done (tokens, answer), the others stay in the list, in order.
    // A piece that holds a zero byte never uses the memo -- neither looked up nor inserted: a slot's words are either still zero or final
    // (an entry never changes once valid), so whatever mixture of old and new words a reader may be handed -- the key and the value are
    // two loads, and a slot can be claimed between them -- a key without zero bytes inside its length can only ever equal a COMPLETE key of the
    // same length, and then the value it is paired with is either that key's (valid) or not valid at all.
    // (r16 / ix / fkq: the entry and the quad of the `take` lanes that hold a NEW entry, fetched together by those very lanes: the memo slot is the only
    //  round trip between taking an entry and answering it.)  Returns, per lane, whether its piece has to be merged; the caller lists it.
    auto memo_phase = [&](int take, uint32_t r16, uint32_t ix, uint4 fkq) -> bool {
        (void)simt::ballot(true);
        const bool mine = lane < take;
        const int si = (int)(ix >> 10), j = (int)(ix & 1023u), rel = (int)(r16 & 1023u), len = (int)((r16 >> 10) & 15u) + 1;
        bool hit = false;
        uint32_t hit_slot = 0;
        uint4 vv; vv.x = vv.y = vv.z = vv.w = 0;
        if (mine && memo) {
            uint32_t kw[4];
            bool nul;
            key_of(fkq, len, kw, &nul);
            const uint32_t b = tkz_mulhi(tkz_hash_memo(kw, (uint32_t)len), T.memo_n / kMemoWays) * kMemoWays;
#pragma unroll
            for (int wy = 0; wy < (int)kMemoWays; ++wy) {
                const TkzMemoSlot* slot = &T.memo[b + wy];
                const uint4 kk = tkz_load16(&slot->k[0]);
                const uint4 v = tkz_load16(&slot->v[0]);
                // (the valid tag is in ALL FOUR value words: a value whose 16-byte store became visible word by word -- nothing in HIP's memory
                //  model says a dwordx4 access is single-copy atomic across CUs / XCDs -- is not valid until its last word is there)
                const bool h = !nul && ((v.x & v.y & v.z & v.w) & kMemoValid) && v.x != kMemoBusy && kk.x == kw[0] && kk.y == kw[1] && kk.z == kw[2] && kk.w == kw[3] &&
                               ((v.y >> 27) & 15u) == (uint32_t)(len - 1);
                if (h) { hit = true; vv = v; hit_slot = b + wy; }
            }
        }
        // A learning batch: in a large batch ONE lane of the wavefront (another one every time) reports its hit -- a sample of one hit in 64 x 8.  Not every hit: the
        // hottest pieces of Zipf-distributed text are hit millions of times a batch, and device-scope atomics on ONE address serialise at about a
        // microsecond each (the first batch under synth100k took 2.4 s instead of 25 ms when every hit of every eighth group was counted).  A counter
        // also stops at kMemoHitsSat (read with an agent-scope atomic load: the line in this XCD's L2 may be stale): such a slot is promoted anyway.
        if (count_hits) {
            if (hit && (!sparse || lane == ((done * 5 + nl0 + nl1) & 63)) && tkz_atomic_load_agent(&T.memo_hits[hit_slot]) < kMemoHitsSat)
                simt::atomic_add(reinterpret_cast<int*>(&T.memo_hits[hit_slot]), 1);
        }
        if (P.stats) { st_look += tkz_popc64(simt::ballot(mine && memo)); st_hit += tkz_popc64(simt::ballot(hit)); }   // (statistics run only: wave-uniform, null in the timed runs)
        const int cnt = hit ? (int)((vv.x >> 29) & 3u) + 1 : 0;
        (void)assign(hit, cnt, si, j, rel);
        if (hit) {                                            // (a memo entry holds <= 4 tokens: they go into the entry's quad)
            uint4 tq; tq.x = vv.x & 0x07FFFFFFu; tq.y = vv.y & 0x07FFFFFFu; tq.z = vv.z & 0x07FFFFFFu; tq.w = vv.w & 0x07FFFFFFu;
            mq0[si * (int64_t)P.mcap + j] = tq;
        }
        (void)simt::ballot(true);
        return mine && !hit;
    };
    // one batch: lane i < n merges the piece of entry i of list c
    auto run_batch = [&](int c, int n) {
        (void)simt::ballot(true);
        int cnt = 0, si = 0, j = 0, rel = 0, e1 = 0, len = 1;
        bool nul = false;
        uint32_t alive = 1;
        uint32_t kw[4] = {0, 0, 0, 0};
        if (lane < n) {
            const uint32_t r16 = s_rec[64 * c + lane], ix = s_idx[64 * c + lane];
            si = (int)(ix >> 10); j = (int)(ix & 1023u); rel = (int)(r16 & 1023u); len = (int)((r16 >> 10) & 15u) + 1;
            key_of(tkz_load16(&mq0[si * (int64_t)P.mcap + j]), len, kw, &nul);
            cnt = tkz_bpe_lane_f<NMAX>(T, kw, len, ids, pr, byte_id, pair_rank, &alive, &e1);
            err |= e1;
        }
        int32_t* dst = assign(lane < n, cnt, si, j, rel);
        if (lane < n) {
            uint32_t t4[4] = {0, 0, 0, 0};
            int i = 0;
            for (uint32_t a = alive; a; a &= a - 1) { const uint32_t t = ids[tkz_ctz32(a)]; if (dst) dst[i] = (int32_t)t; if (i < 4) { if (i == 0) t4[0] = t; else if (i == 1) t4[1] = t; else if (i == 2) t4[2] = t; else t4[3] = t; } ++i; }
            if (cnt <= 4) { uint4 tq; tq.x = t4[0]; tq.y = t4[1]; tq.z = t4[2]; tq.w = t4[3]; mq0[si * (int64_t)P.mcap + j] = tq; }
            // a piece of <= 4 tokens takes a memo slot of its bucket if one is free (an entry is never replaced: a hit stays valid for good)
            if (memo && cnt <= 4 && !e1 && !nul) {
                const uint32_t b = tkz_mulhi(tkz_hash_memo(kw, (uint32_t)len), T.memo_n / kMemoWays) * kMemoWays;
                bool placed = false;
#pragma unroll
                for (int wy = 0; wy < (int)kMemoWays; ++wy) {
                    TkzMemoSlot* slot = &T.memo[b + wy];
                    // (a plain load first: a piece that lost its slot to another one comes back millions of times on repetitive text, and a
                    //  failing compare-and-swap is still an atomic on one hot address)
                    if (!placed && *reinterpret_cast<volatile uint32_t*>(&slot->v[0]) == 0u && simt::atomic_cas(&slot->v[0], 0u, kMemoBusy) == 0u) {
                        // The key and the value are one 16-byte store each, and there is NO fence between or behind them.  The protocol does
                        // not rely on those stores (or a reader's 16-byte loads) being single-copy atomic: EVERY value word carries the valid
                        // tag (bit 31), so a value is accepted only when all four words are the new ones -- any mixture with the old words
                        // (zero, or BUSY in v[0]) is a miss --, and then its length field is the key's; a key seen word by word is a mixture of
                        // the new words and zero words, and a looked-up piece (no zero byte inside its length) can equal such a mixture only
                        // if the missing words lie beyond its length -- where the complete key is zero too: every mixture is a miss or the
                        // right hit, in whatever order the eight words become visible.  (A device-scope release fence here wrote the XCD's dirty L2 lines back for EVERY insertion: the
                        // first batch on an empty memo with many misses -- 369 M short misses of the held-out vocabulary -- spent 566 ms
                        // in this kernel, ten times what it takes with the memo switched off.)
                        uint4 kk; kk.x = kw[0]; kk.y = kw[1]; kk.z = kw[2]; kk.w = kw[3];
                        *reinterpret_cast<uint4*>(&slot->k[0]) = kk;
                        uint4 nv; nv.x = kMemoValid | ((uint32_t)(cnt - 1) << 29) | t4[0]; nv.y = kMemoValid | ((uint32_t)(len - 1) << 27) | t4[1]; nv.z = kMemoValid | t4[2]; nv.w = kMemoValid | t4[3];
                        *reinterpret_cast<uint4*>(&slot->v[0]) = nv;
                        placed = true;
                    }
                }
            }
        }
        (void)simt::ballot(true);
    };
    (void)simt::ballot(true);
    // Entry g of the group's concatenated lists is entry g - pre[q] of sub-tile q.  Lane i always has entry done + i of the lists in flight
    // (entry, quad: two independent loads), requested while the entries before them are looked up in the memo.
    auto request = [&](int g, uint32_t* r16, uint32_t* ix, uint4* kq) {
        *r16 = 0; *ix = 0; kq->x = kq->y = kq->z = kq->w = 0;
        if (g < ntotal) {
            const int q = tkz_find_list<kGroup>(s_pre, g), j = g - (int)s_pre[q];
            const uint32_t ent = tkz_load_nt(&ml0[q * (int64_t)P.mcap + j]);
            *kq = tkz_load16(&mq0[q * (int64_t)P.mcap + j]);
            *r16 = (ent & 1023u) | (((ent >> kMrLenShift) & 15u) << 10);
            *ix = (uint32_t)((q << 10) | j);
        }
    };
    // The pieces that have to be merged wait in TWO lists, by length (round 6): a batch lasts as long as its longest piece -- a merge a step, a round trip a
    // merge --, and with lengths 1..16 in one batch the lanes of the short pieces idled for half of it (lane use 0.4).  A list that reaches 64 entries is
    // merged; what is left of both at the end goes as ONE batch if it fits one (the bench text: ~40 survivors a group), else as one batch a list.
    // (Two lists only for a group with many misses -- kMsTwoListsMin entries, 20 a sub-tile: source text has ~860 a group and gains (k_merge_short 1.66 -> 1.10 ms on
    //  436 MB), the bench text has ~160, ends with ONE batch of ~40 pieces either way and only paid for the second list: 2.39 -> 2.55 ms.  profiles/r06/variants_merge_short2.txt)
    const bool two = ntotal >= kMsTwoListsMin;
    uint32_t a_r16, a_ix;
    uint4 a_kq;
    request(lane, &a_r16, &a_ix, &a_kq);
    while (done < ntotal) {
        const int take = ntotal - done < 64 ? ntotal - done : 64;
        const uint32_t f_r16 = a_r16, f_ix = a_ix;
        const uint4 f_kq = a_kq;
        done += take;
        request(done + lane, &a_r16, &a_ix, &a_kq);            // (the entries behind these: in flight during the memo lookups)
        const bool merge_it = memo_phase(take, f_r16, f_ix, f_kq);
        const int cls = two && ((f_r16 >> 10) & 15u) >= (uint32_t)kMsShortLen ? 1 : 0;       // (the field holds len - 1)
#pragma unroll 1
        for (int c = 0; c < 2; ++c) {
            const uint64_t m = simt::ballot(merge_it && cls == c);
            const int had = c ? nl1 : nl0;
            const int pos = had + tkz_popc64(m & tkz_lowmask(lane)), tot = had + tkz_popc64(m);
            const bool here = merge_it && cls == c;
            if (here && pos < 64) { s_rec[64 * c + pos] = (uint16_t)f_r16; s_idx[64 * c + pos] = (uint16_t)f_ix; }
            if (tot >= 64) {                                   // the list is full: its batch, then the entries that did not fit
                run_batch(c, 64);
                if (here && pos >= 64) { s_rec[64 * c + pos - 64] = (uint16_t)f_r16; s_idx[64 * c + pos - 64] = (uint16_t)f_ix; }
                if (c) nl1 = tot - 64; else nl0 = tot - 64;
            } else if (c) nl1 = tot; else nl0 = tot;
        }
    }
    if (nl0 + nl1 <= 64 && nl1 > 0) {                           // (one batch for both lists' leftovers)
        (void)simt::ballot(true);
        if (lane < nl1) { s_rec[nl0 + lane] = s_rec[64 + lane]; s_idx[nl0 + lane] = s_idx[64 + lane]; }
        nl0 += nl1; nl1 = 0;
    }
#pragma unroll 1
    for (int c = 0; c < 2; ++c) { const int n = c ? nl1 : nl0; if (n > 0) run_batch(c, n); }
    (void)simt::ballot(true);
    // tokens of every sub-tile of the group: one per piece, plus what the merges added (k_merge_long adds its own later)
    if (lane < kGroup && sub0 + lane < P.nsub) {
        const int tc = my_np + s_extra[lane] + (P.pextra ? P.pextra[sub0 + lane] : 0);
        if (P.tc_atomic) simt::atomic_add(&P.tile_count[sub0 + lane], tc);            // (the long pieces' kernels run beside this one and add theirs: k_probe has zeroed the counts)
        else P.tile_count[sub0 + lane] = tc;
    }
    if (err) simt::atomic_or((unsigned*)&P.counters[0], (unsigned)err);
    if (P.stats && lane == 0 && st_look) { simt::atomic_add64(&P.stats[0], (unsigned long long)st_look); simt::atomic_add64(&P.stats[1], (unsigned long long)st_hit); }
}
// (LDS: 4 x 9.5 KB of merge state + 0.5 KB = 38.5 KB per workgroup, and <= 128 VGPRs: four workgroups = 16 wavefronts per CU)
// A batch whose miss lists or record buffer turned out too small (k_probe / k_list_stats flag it) is run again by the host with larger ones: the
// kernels behind those two have nothing to add to an attempt that is thrown away, and on a fresh encoder's first miss-heavy batch that attempt was
// costing as much as the one that counts.
TKZ_DEV bool tkz_attempt_failed(const EncodeParams& P) { return (P.counters[0] & (kErrMissCap | kErrCapacity)) != 0; }

TKZ_KERNEL_OCC(kMsThreads, 4) void k_merge_short(TkzTables T, EncodeParams P) {
    if (tkz_attempt_failed(P)) return;
    TKZ_SHARED uint4 s_wave[kMsThreads / 64][kMsLdsQuads];
    TKZ_SHARED uint16_t s_brank16[256];
    tkz_ms_brank_init(T, s_brank16);
    simt::sync();
    const int64_t grp = tkz_xcd_block(simt::bid(), simt::nblocks()) * (kMsThreads / 64) + simt::wave();
    tkz_merge_short_group(T, P, grp, tkz_ms_lds(s_wave[simt::wave()], s_brank16));
}

// The pieces of 17..256 bytes that have to be merged (longer ones: k_merge_coop below), and the token counts of the giant ones.  One lane per piece with its state in a
// span of an LDS arena sized for it (tkz_bpe_lane_u up to 64 bytes; tkz_bpe_lane_varc / _var beyond: pair ranks [| ids] [| alive bits], preceded by the piece's bytes).
// The long-miss lists of the 64 sub-tiles of a chunk are walked as one list, kLongSeg entries at a time, and every such segment is
// SORTED BY LENGTH (a counting sort over 16 length classes, in LDS) before it is cut into batches of up to 64 lanes: a merge costs a scan
// over the whole piece and a piece of n bytes takes ~n/2 of them, so a 60-byte piece is ten times the work of a 17-byte one -- in list
// order a batch took as long as its longest piece while the other lanes idled (33 % of the lanes active on CJK text).  Spans are padded to
// an odd number of 16-byte quads: pieces of one class have equal spans, and with an even quad stride their 16-byte reads collide.
// A chunk = 64 consecutive sub-tiles (one per lane: their long-miss lists walked as one list).  Until round 5 a chunk was the unit of work a wavefront
// takes; REAL text showed what that costs: its long pieces are not spread evenly -- one file of CJK prose is 64 KiB after 64 KiB of nothing but 100..250-byte
// pieces, ~10 ms of merging for the ONE wavefront that owns such a chunk while the other 3,000 have long finished (k_merge_long 13 ms of a 17 ms step on
// 436 MB of source text, for 0.3 ms of work).  Smaller chunks cut that tail and cost sparse text its lane fill (16 sub-tiles: the headline workload's one
// long miss per KiB makes batches of 16 lanes instead of 64, k_merge_long 1.4 -> 3.7 ms).  So: a chunk whose lists hold more than kLongDense entries is
// split into kLongParts units of work, a sparse one stays whole.
#ifndef TKZ_LONG_PARTS
#define TKZ_LONG_PARTS 4
#endif
#ifndef TKZ_LONG_DENSE
#define TKZ_LONG_DENSE 192
#endif
constexpr int kLongParts = TKZ_LONG_PARTS, kLongDense = TKZ_LONG_DENSE;
static_assert(kLongParts >= 1 && kLongParts <= 64 && 64 % kLongParts == 0, "a part is a whole number of the chunk's 64 sub-tiles");
constexpr int kLongSeg = 384;
constexpr int kFastPiece = 64;           // long misses of up to this many bytes: the fast batches of k_merge_long (tkz_bpe_lane_u)
static_assert(kFastPiece <= kLanePiece && kFastPiece <= kSmallLanePiece, "every caller's lane limit covers the fast batches");
constexpr int kLenClasses = 16;
TKZ_HD int tkz_len_class(int len) {          // 17..1024, monotone
    if (len <= 32) return (len - 17) >> 2;               // 17-20, 21-24, 25-28, 29-32
    if (len <= 64) return 4 + ((len - 33) >> 3);         // 33-40, 41-48, 49-56, 57-64
    if (len <= 128) return len <= 96 ? 8 : 9;
    if (len <= 256) return len <= 192 ? 10 : 11;
    if (len <= 512) return len <= 384 ? 12 : 13;
    return len <= 768 ? 14 : 15;
}
// LDS of the wavefront of k_merge_long
struct LongLds { uint32_t* arena; int arena_dwords; int* pre; int* cls; uint16_t* ord; int32_t* brank; };
constexpr int kLongLdsBytes = kArenaDwords * 4 + 4 * 68 + 4 * kLenClasses + 2 * kLongSeg + 4 * 256;
constexpr int kLongLdsQuads = (kLongLdsBytes + 15) / 16;
TKZ_DEV LongLds tkz_long_lds(uint4* quads) {
    LongLds L;
    uint8_t* b = reinterpret_cast<uint8_t*>(quads);
    L.arena = reinterpret_cast<uint32_t*>(b); b += kArenaDwords * 4; L.arena_dwords = kArenaDwords;
    L.brank = reinterpret_cast<int32_t*>(b); b += 4 * 256;                    // id of every single byte: in LDS, not a gather per byte
    L.pre = reinterpret_cast<int*>(b); b += 4 * 68;
    L.cls = reinterpret_cast<int*>(b); b += 4 * kLenClasses;
    L.ord = reinterpret_cast<uint16_t*>(b);                                   // the segment's list positions, by length class
    return L;
}
TKZ_DEV void tkz_long_brank_init(const TkzTables& T, int32_t* s_brank) {     // by one wavefront
    for (int i = simt::lane(); i < 256; i += 64) s_brank[i] = T.byte_rank[i];
    (void)simt::ballot(true);
}
// The development counters of the long-miss kernels (make DEVPROF=1, TKZ_DEV_ABLATE bit 4): clock ticks of a wavefront by phase, batches, lanes, merges
struct LongProf {
    bool on = false;
    long long t[6] = {0, 0, 0, 0, 0, 0};            // sort / queue | batch formation | bytes | first level | merges | emission and answers
    long long batches = 0, lanes = 0, steps = 0, merges = 0, units = 0, t0 = 0, begin = 0;
};
#ifdef TKZ_DEVPROF
#define TKZ_PF_MARK(i) do { if (PF.on) { const long long pf_now = simt::clock(); PF.t[i] += pf_now - PF.t0; PF.t0 = pf_now; } } while (0)
TKZ_DEV void tkz_long_prof_begin(const EncodeParams& P, LongProf& PF) { PF.on = TKZ_DEV_FLAG(P, 16) && P.devprof; if (PF.on) PF.begin = PF.t0 = simt::clock(); }
TKZ_DEV void tkz_long_prof_end(const EncodeParams& P, LongProf& PF) {
    if (!PF.on) return;
    int mt;
    (void)tkz_wave_scan_sum((int)PF.merges, &mt);
    if (simt::lane() == 0) {
        simt::atomic_add64(&P.devprof[32], 1); simt::atomic_add64(&P.devprof[33], (unsigned long long)(simt::clock() - PF.begin));
        for (int i = 0; i < 6; ++i) simt::atomic_add64(&P.devprof[34 + i], (unsigned long long)PF.t[i]);
        simt::atomic_add64(&P.devprof[40], (unsigned long long)PF.batches); simt::atomic_add64(&P.devprof[41], (unsigned long long)PF.lanes);
        simt::atomic_add64(&P.devprof[42], (unsigned long long)PF.steps); simt::atomic_add64(&P.devprof[43], (unsigned long long)mt);
        simt::atomic_add64(&P.devprof[44], (unsigned long long)PF.units);
    }
}
#else
#define TKZ_PF_MARK(i) do { } while (0)
TKZ_DEV void tkz_long_prof_begin(const EncodeParams&, LongProf&) {}
TKZ_DEV void tkz_long_prof_end(const EncodeParams&, LongProf&) {}
#endif
// ONE BATCH of long misses: the lanes for which `valid` holds (a prefix of the wavefront, lane 0 among them) each bring a piece -- entry j of sub-tile
// sub's long list, len bytes at byte rel of the sub-tile -- in ascending order of tkz_len_class.  Merges a prefix of them, one piece a lane, answers their
// list entries and returns how many it took (>= 1); the caller comes back with the rest.  (COMPACT: ranks below 2^21, i.e. every published vocabulary.)
// (on_limit(n): called as soon as the number of pieces the batch takes is known, before anything is merged -- the queue form requests its next entries there)
template <bool COMPACT, class OnLimit>
TKZ_DEV int tkz_long_batch(const TkzTables& T, const EncodeParams& P, const LongLds& LD, bool valid, int64_t sub, int j, int rel, int len, int lane_piece, int& err, LongProf& PF, OnLimit on_limit) {
    uint32_t* s_arena = LD.arena;
    const int32_t* s_brank = LD.brank;
    const int lane = simt::lane();
    constexpr bool compact = COMPACT;                           // no ids[] array (tkz_bpe_lane_varc): 40 % more pieces per batch
    const int64_t abs = sub * kSub + rel;
    const int64_t lidx = sub * (int64_t)P.mcap + (P.mcap - 1 - j);     // the piece's list entry (and quad)
    bool log_it = false;                             // (a learning batch: this lane's piece goes into the log below)
    uint4 log_tok; log_tok.x = log_tok.y = log_tok.z = log_tok.w = 0;
    int log_cnt = 0;
    const uint32_t* log_bw = s_arena;                // the piece's bytes in the arena
    int limit;
    // ---- a FAST batch (round 6): the next pieces of up to 32 (else: up to 64) bytes, every one in a span of the size the longest of them
    //      needs, merged by tkz_bpe_lane_u (tkz_bpe.h).  The positions are sorted by length class and 32 | 33, 64 | 65 are class edges,
    //      so the pieces of a batch are a prefix of the lanes.
    const int len0 = simt::first_lane(len);          // (lane 0 always holds a piece)
    if (COMPACT && len0 <= kFastPiece) {           // (kFastPiece <= lane_piece: static_assert below)
        const int cut = len0 <= 32 ? 32 : kFastPiece;
        const int nok = tkz_ctz64z(~simt::ballot(valid && len <= cut));
        const int maxlen = (int)~simt::wave_min_u32(~(uint32_t)(lane < nok ? len : 0));
        const int nq = (maxlen + 3) >> 2;            // dwords of bytes = quads of pair keys, the same for every piece of the batch
        const int nbd = (nq + 3) & ~3;
        const int spanq = ((nbd >> 2) + nq) | 1;     // an odd number of quads: the spans' 16-byte reads then sit on distinct banks
        const int fit = (LD.arena_dwords / 4) / spanq; // (>= 1: the arena covers a piece of lane_piece bytes)
        limit = nok < fit ? nok : fit;
        on_limit(limit);
        TKZ_PF_MARK(1);
#ifdef TKZ_DEVPROF
        int pf_mg = 0;
#endif
        if (lane < limit) {
            uint32_t* bw = s_arena + lane * (spanq * 4);
            log_bw = bw;
            {   // nbd dwords of text from the piece's first byte on (past its end: whatever follows; past the end of the text: 0): every load is requested
                // before the first is used (a loop over the dwords waited for one round trip to the text after the other)
                const int64_t a0 = abs & ~(int64_t)3;
                const uint32_t sh = (uint32_t)(abs & 3) * 8u;
                auto fetch = [&](auto NDW) {
                    constexpr int ND = decltype(NDW)::value;
                    uint32_t t[ND + 1];
                    if (a0 + 4 * (int64_t)(ND + 1) <= P.total) {
#pragma unroll
                        for (int w = 0; w <= ND; ++w) t[w] = *reinterpret_cast<const uint32_t*>(P.bytes + a0 + 4 * w);
                    } else {
                        for (int w = 0; w <= ND; ++w) {
                            uint32_t v = 0;
                            for (int b = 0; b < 4; ++b) if (a0 + 4 * w + b < P.total) v |= (uint32_t)P.bytes[a0 + 4 * w + b] << (8 * b);
                            t[w] = v;
                        }
                    }
                    uint4* bw4 = reinterpret_cast<uint4*>(bw);
#pragma unroll
                    for (int g = 0; g < ND / 4; ++g)
                        if (4 * g < nbd) {                  // (wave-uniform)
                            uint4 v;
                            v.x = simt::alignbit(t[4 * g + 1], t[4 * g], sh); v.y = simt::alignbit(t[4 * g + 2], t[4 * g + 1], sh);
                            v.z = simt::alignbit(t[4 * g + 3], t[4 * g + 2], sh); v.w = simt::alignbit(t[4 * g + 4], t[4 * g + 3], sh);
                            bw4[g] = v;
                        }
                };
                if (cut == 32) fetch(std::integral_constant<int, 8>{}); else fetch(std::integral_constant<int, 16>{});
            }
            uint32_t* pr = bw + nbd;
            uint32_t q4[4];
            int e1 = 0, cnt;
            TKZ_PF_MARK(2);
            tkz_bpe_lane_u_init(T, bw, len, nq, pr);
            TKZ_PF_MARK(3);
            if (cut == 32) {
                uint32_t alive;
                cnt = tkz_bpe_lane_u_merge<uint32_t>(T, bw, len, nq, pr, s_brank, &alive);
                TKZ_PF_MARK(4);
                tkz_bpe_lane_u_emit<uint32_t>(bw, len, nq, pr, s_brank, alive, cnt > 4, P.tmp + abs, q4, &e1);
            } else {
                uint64_t alive;
                cnt = tkz_bpe_lane_u_merge<uint64_t>(T, bw, len, nq, pr, s_brank, &alive);
                TKZ_PF_MARK(4);
                tkz_bpe_lane_u_emit<uint64_t>(bw, len, nq, pr, s_brank, alive, cnt > 4, P.tmp + abs, q4, &e1);
            }
            err |= e1;
#ifdef TKZ_DEVPROF
            pf_mg = len - cnt;
#endif
            // (five tokens and more wait in tmp at the piece's position; up to four go into the entry's quad, where k_place finds them in the
            //  round trip that fetches the answers)
            if (cnt <= 4) {
                uint4 tq; tq.x = q4[0]; tq.y = q4[1]; tq.z = q4[2]; tq.w = q4[3];
                P.mquad[lidx] = tq;
                P.mlist[lidx] = tkz_result_inline(cnt);
                if (P.long_log && len <= kLongLogMaxLen && !e1 && (!P.long_log_sparse || ((sub >> 6) & 7) == 0)) { log_it = true; log_tok = tq; log_cnt = cnt; }
            } else P.mlist[lidx] = tkz_result_entry(false, cnt, rel);
            if (cnt > 1) simt::atomic_add(&P.tile_count[sub], cnt - 1);
        }
        TKZ_PF_MARK(5);
#ifdef TKZ_DEVPROF
        if (PF.on) {
            PF.merges += pf_mg;                                        // (per lane; summed over the wave at the end)
            const int mx = (int)~simt::wave_min_u32(~(uint32_t)pf_mg);
            if (lane == 0) { ++PF.batches; PF.lanes += limit; PF.steps += mx; }
        }
#endif
    } else {
    // ---- the general batch: pieces of more than kFastPiece bytes (and every piece of a vocabulary with ranks of 2^21 and more), each in a span of
    //      its own size, up to the first whose state no longer fits the arena
    const int nbw = (len + 3) >> 2;
    const bool mine = valid && len <= lane_piece;    // (a longer piece keeps its entry as it is: k_merge_coop answers it -- k_probe has flagged its sub-tile)
    int need = 0;
    if (mine) {
        need = ((nbw + 3) & ~3) + (compact ? tkz_bpe_varc_dwords(len) : tkz_bpe_var_dwords(len));
        if (!((need >> 2) & 1)) need += 4;           // an odd number of quads: equal spans then sit on distinct banks
    }
    int btot;
    const int aoff = tkz_wave_scan_sum(need, &btot);
    const uint64_t bad = simt::ballot(mine && aoff + need > LD.arena_dwords);
    limit = bad ? tkz_ctz64(bad) : 64;               // lanes at or beyond `limit` wait for the next batch (limit >= 1: one piece always fits)
    on_limit(limit);
    if (mine && lane < limit) {
        uint32_t* bw = &s_arena[aoff];                   // (len + 3) / 4 dwords of bytes, then the merge state
        log_bw = bw;
        {
            const int64_t a0 = abs & ~(int64_t)3;
            const uint32_t sh = (uint32_t)(abs & 3) * 8u;
            uint32_t prev = 0;
            if (a0 + 4 <= P.total) prev = *reinterpret_cast<const uint32_t*>(P.bytes + a0);
            else for (int b = 0; b < 4; ++b) if (a0 + b < P.total) prev |= (uint32_t)P.bytes[a0 + b] << (8 * b);
            for (int w = 0; w < nbw; ++w) {
                const int64_t p = a0 + 4 * (w + 1);
                uint32_t nx = 0;
                if (p + 4 <= P.total) nx = *reinterpret_cast<const uint32_t*>(P.bytes + p);
                else for (int b = 0; b < 4; ++b) if (p + b < P.total) nx |= (uint32_t)P.bytes[p + b] << (8 * b);
                bw[w] = simt::alignbit(nx, prev, sh);
                prev = nx;
            }
        }
        const uint8_t* pbytes = reinterpret_cast<const uint8_t*>(bw);
        uint32_t* st = bw + ((nbw + 3) & ~3);             // (the state arrays are read 16 bytes at a time)
        auto at = [&](int i) -> uint32_t { return pbytes[i]; };
        int e1 = 0, cnt;
        if constexpr (COMPACT) {
            cnt = tkz_bpe_lane_varc(T, at, len, st, &e1, s_brank); tkz_bpe_varc_emit(at, st, len, s_brank, P.tmp + abs);
        } else {
            cnt = T.max_rank <= kVarPackedMaxRank ? tkz_bpe_lane_var<true>(T, at, len, st, &e1, s_brank) : tkz_bpe_lane_var<false>(T, at, len, st, &e1, s_brank);
            tkz_bpe_var_emit(st, len, P.tmp + abs);
        }
        err |= e1;
        // (the tokens are in tmp at the piece's position; up to four also go into the entry's quad, where k_place finds them
        //  in the round trip that fetches the answers)
        if (cnt <= 4) {
            const int32_t* tk = P.tmp + abs;
            uint4 tq; tq.x = (uint32_t)tk[0]; tq.y = cnt > 1 ? (uint32_t)tk[1] : 0u; tq.z = cnt > 2 ? (uint32_t)tk[2] : 0u; tq.w = cnt > 3 ? (uint32_t)tk[3] : 0u;
            P.mquad[lidx] = tq;
            P.mlist[lidx] = tkz_result_inline(cnt);
            if (P.long_log && len <= kLongLogMaxLen && !e1 && (!P.long_log_sparse || ((sub >> 6) & 7) == 0)) { log_it = true; log_tok = tq; log_cnt = cnt; }
        } else P.mlist[lidx] = tkz_result_entry(false, cnt, rel);
        if (cnt > 1) simt::atomic_add(&P.tile_count[sub], cnt - 1);
    }
    }
    if (P.long_log) {                                // (wave-uniform; a learning batch only) one atomic for the wavefront's records
        int ltot;
        const int lpre = tkz_wave_scan_sum(log_it ? 1 : 0, &ltot);
        unsigned long long lbase = 0;
        if (lane == 0 && ltot) lbase = simt::atomic_add64(P.long_log_count, (unsigned long long)ltot);
        lbase = ((unsigned long long)simt::shflu((uint32_t)(lbase >> 32), 0) << 32) | simt::shflu((uint32_t)lbase, 0);
        if (log_it && lbase + (unsigned long long)lpre < (unsigned long long)P.long_log_cap) {
            uint32_t* rec = P.long_log + (lbase + (unsigned long long)lpre) * kLongLogDwords;
            for (int w = 0; w < 7; ++w) {                    // (the piece's bytes, still in the arena)
                const int nbz = len - 4 * w;
                rec[w] = nbz <= 0 ? 0u : (nbz >= 4 ? log_bw[w] : (log_bw[w] & ((1u << (8 * nbz)) - 1u)));
            }
            rec[7] = (uint32_t)len | ((uint32_t)log_cnt << 8);
            rec[8] = log_tok.x; rec[9] = log_tok.y; rec[10] = log_tok.z; rec[11] = log_tok.w;
        }
    }
    (void)simt::ballot(true);
    return limit;
}
// chunks c0, c0 + cstep, ... of 64 sub-tiles each, by one wavefront
// (COMPACT: ranks below 2^21, i.e. every published vocabulary -- no ids[] array)
template <bool COMPACT, int PARTS = kLongParts, int DENSE = kLongDense>
// (lane_piece: pieces of up to this many bytes are merged here -- kLanePiece on the batch path, which has k_merge_coop for the longer ones; the
//  single-launch kernel has no such kernel and takes kSmallLanePiece)
TKZ_DEV void tkz_merge_long_chunks(const TkzTables& T, const EncodeParams& P, int64_t c0, int64_t cstep, const LongLds& LD, const int lane_piece = kLanePiece) {
    int* s_pre = LD.pre;
    int* s_cls = LD.cls;
    uint16_t* s_ord = LD.ord;
    const int lane = simt::lane();
    int err = 0;
    LongProf PF;
    tkz_long_prof_begin(P, PF);
    // A unit of work = a chunk of 64 sub-tiles, or -- when the chunk's lists hold more than kLongDense entries -- one of its kLongParts parts
    // (the parts of a sparse chunk other than part 0 have nothing to do).
    // (part-major: units 0 .. nchunks-1 are part 0 of every chunk.  Chunk-major -- unit u = part u % 4 of chunk u / 4 -- put the only units that have
    //  work in sparse text, the parts 0, on workgroups 0, 4, 8 ...: workgroups go round the 8 XCDs, so two of them did everything, 1.4 -> 5 ms.)
    const int64_t nchunks = (P.nsub + 63) / 64;
    for (int64_t u = c0; u < nchunks * PARTS; u += cstep) {
        const int64_t c = u % nchunks;
        const int part = (int)(u / nchunks);
        const int64_t t = c * 64 + lane;
        int my_nl = 0;
        if (t < P.nsub) {
            const uint32_t mc = P.mcount[t];
            my_nl = (int)(mc >> 16);
            if ((int)(mc & 0xFFFFu) + my_nl > P.mcap) my_nl = 0;               // (cut list: reported by k_probe, the batch is redone)
            // the giant piece of the sub-tile (its last piece): merged by k_giant_merge, its token count is added here (by the chunk's part 0)
            if (part == 0 && (P.heavy_flag[t] & 2u)) { const int g = P.giant_cnt[t]; if (g > 1) simt::atomic_add(&P.tile_count[t], g - 1); }   // (< 0: no pool, the call is retried)
        }
        int ntotal;
        (void)tkz_wave_scan_sum(my_nl, &ntotal);
        if (ntotal > DENSE) { if (lane / (64 / PARTS) != part) my_nl = 0; }      // dense: this unit's share of the sub-tiles
        else if (part != 0) continue;                                                    // sparse: the whole chunk is part 0's
        const int pre = tkz_wave_scan_sum(my_nl, &ntotal);
        if (!ntotal) continue;
        (void)simt::ballot(true);
        s_pre[lane] = pre;
        if (lane == 0) s_pre[64] = ntotal;
        (void)simt::ballot(true);
        // position g of the 64 lists taken as one: entry g - pre[q] (from the back) of sub-tile q
        auto entry_at = [&](int g, int* q, int* j) -> uint32_t {
            *q = tkz_find_list<64>(s_pre, g); *j = g - s_pre[*q];
            return tkz_load_nt(&P.mlist[(c * 64 + *q) * (int64_t)P.mcap + (P.mcap - 1 - *j)]);
        };
#ifdef TKZ_DEVPROF
        if (PF.on) { ++PF.units; PF.t0 = simt::clock(); }
#endif
        for (int seg0 = 0; seg0 < ntotal; seg0 += kLongSeg) {
            const int nseg = ntotal - seg0 < kLongSeg ? ntotal - seg0 : kLongSeg;
            // ---- counting sort of the segment's positions by length class ----
            if (lane < kLenClasses) s_cls[lane] = 0;
            (void)simt::ballot(true);
            uint32_t mycls = 0;                                  // the classes of this lane's (up to 8) entries, 4 bits each
#pragma unroll
            for (int i = 0; i < kLongSeg / 64; ++i) {
                const int e = lane + 64 * i;
                if (e < nseg) {
                    int q, j;
                    const uint32_t ent = entry_at(seg0 + e, &q, &j);
                    const int cl = tkz_len_class((int)((ent >> kMrLenShift) & 1023u) + 1);
                    mycls |= (uint32_t)cl << (4 * i);
                    simt::atomic_add(&s_cls[cl], 1);
                }
            }
            (void)simt::ballot(true);
            {
                int tot;
                const int v = lane < kLenClasses ? s_cls[lane] : 0;
                const int x = tkz_wave_scan_sum(v, &tot);
                (void)simt::ballot(true);
                if (lane < kLenClasses) s_cls[lane] = x;
            }
            (void)simt::ballot(true);
#pragma unroll
            for (int i = 0; i < kLongSeg / 64; ++i) {
                const int e = lane + 64 * i;
                if (e < nseg) s_ord[simt::atomic_add(&s_cls[(mycls >> (4 * i)) & 15u], 1)] = (uint16_t)e;
            }
            (void)simt::ballot(true);
            TKZ_PF_MARK(0);
            // ---- batches: the next sorted positions, one per lane, up to the first whose state no longer fits the arena ----
            for (int done = 0; done < nseg;) {
                const bool valid = done + lane < nseg;
                int q = 0, j = 0, len = 1, rel = 0;
                if (valid) {
                    const uint32_t ent = entry_at(seg0 + (int)s_ord[done + lane], &q, &j);
                    rel = (int)(ent & 1023u); len = (int)((ent >> kMrLenShift) & 1023u) + 1;
                }
                const int64_t sub = c * 64 + q;
                const int limit = tkz_long_batch<COMPACT>(T, P, LD, valid, sub, j, rel, len, lane_piece, err, PF, [](int) {});
                (void)simt::ballot(true);
                done += limit < nseg - done ? limit : nseg - done;
            }
        }
    }
    if (err) simt::atomic_or((unsigned*)&P.counters[0], (unsigned)err);
    tkz_long_prof_end(P, PF);
}
// (a small batch -- TKZ_OPT_LATENCY_BYTES --, where the call waits for the slowest wavefront: k_merge_latency's unit of work is 4 sub-tiles whatever their lists
//  hold -- ~20 entries of ordinary text, one batch of lanes -- instead of up to 64 sub-tiles and five batches one after the other: 93 us of a 1 MB call)
constexpr int kLongPartsLatency = 16;

// ---- The long misses of a LARGE batch, binned by length class ACROSS the batch (round 6) ----------------------------------------------------------
// The chunk form above forms its batches inside one unit of work (a chunk of 64 sub-tiles or a quarter of it): on mixed text that is ~290 entries cut
// by length class into seven batches of 41 lanes on average (the development counters: lanes/batch 40.7 of 64), and a file of CJK prose in real text is
// a few chunks that keep their wavefronts for milliseconds.  Here the entries of the WHOLE batch are binned first:
//   k_long_count    per chunk of 64 sub-tiles, the number of its long misses in each of the 16 length classes -> lq_cnt[class * nchunks + chunk]
//   (scan)          exclusive scan of lq_cnt in that order = class-major: all entries of class 0, chunk after chunk, then class 1, ...
//   k_long_scatter  every entry to its place in the queue:  lq[] = sub-tile << 30 | index in its long list << 20 | (len - 1) << 10 | byte in the sub-tile
//   k_merge_long_q  a wavefront takes RANGES of kLqRange queue entries (kLqRangeLong beyond kFastPiece bytes) -- the longest classes first -- and merges them (tkz_long_batch):
//                   full batches of ONE length class, whichever chunks the pieces come from; the work is dealt out 256 pieces at a time, not by chunk.
// No atomics on shared counters (the two passes over the lists cost ~0.1 ms a GB of mixed text); a small batch (TKZ_OPT_LATENCY_BYTES) and the
// single-launch kernel keep the chunk form: three more launches are 15 us.
constexpr int kLqRange = 256, kLqRangeLong = 16;
#ifndef TKZ_QARENA_DWORDS
#define TKZ_QARENA_DWORDS 2304
#endif
constexpr int kQArenaDwords = TKZ_QARENA_DWORDS;   // the arena of k_merge_long_q
static_assert(kQArenaDwords % 4 == 0 && kQArenaDwords >= (kLanePiece + 3) / 4 + 8 + 2 * kLanePiece + 16, "a piece of kLanePiece bytes fits the arena in every form");
#ifdef TKZ_HOSTEMU
constexpr int kLongQGrid = 8;           // (the CPU emulator pays for every idle workgroup)
#else
constexpr int kLongQGrid = 8192;        // wavefronts of k_merge_long_q (13 fit a CU: 3,328 run at once; the ranges beyond are taken round-robin)
#endif
// the entries of chunk c's long lists that a lane merges (<= lane_piece bytes), lane = sub-tile: f(list index j, entry)
template <class F>
TKZ_DEV void tkz_long_walk(const EncodeParams& P, int64_t c, int lane_piece, F f) {
    const int64_t t = c * 64 + simt::lane();
    int nl = 0;
    if (t < P.nsub) {
        const uint32_t mc = P.mcount[t];
        nl = (int)(mc >> 16);
        if ((int)(mc & 0xFFFFu) + nl > P.mcap) nl = 0;                         // (cut list: reported by k_list_stats, the batch is redone)
    }
    // (four entries a step, their loads requested together: a list is read from its end down, one entry a round trip otherwise)
    const uint32_t* top = &P.mlist[t * (int64_t)P.mcap + (P.mcap - 1)];
    for (int j = 0; j < nl; j += 4) {
        uint32_t ent[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) ent[k] = j + k < nl ? tkz_load_nt(top - (j + k)) : 0xFFFFFFFFu;        // (0xFFFFFFFF: 1024 bytes, no lane's piece)
#pragma unroll
        // (an entry that is answered already is k_merge_coop's, which may run BEFORE or beside this walk -- launch_encode --: its length was above lane_piece)
        for (int k = 0; k < 4; ++k) if (j + k < nl && !(ent[k] & kMrDone) && (int)((ent[k] >> kMrLenShift) & 1023u) + 1 <= lane_piece) f(t, j + k, ent[k]);
    }
}
TKZ_KERNEL(256) void k_long_count(EncodeParams P) {
    if (tkz_attempt_failed(P)) return;
    TKZ_SHARED int s_hist[4][kLenClasses];
    const int lane = simt::lane(), wave = simt::wave();
    const int64_t nchunks = (P.nsub + 63) / 64;
    for (int64_t c = simt::bid() * 4 + wave; c < nchunks; c += simt::nblocks() * 4) {
        if (lane < kLenClasses) s_hist[wave][lane] = 0;
        (void)simt::ballot(true);
        tkz_long_walk(P, c, P.lane_piece, [&](int64_t, int, uint32_t ent) { simt::atomic_add(&s_hist[wave][tkz_len_class((int)((ent >> kMrLenShift) & 1023u) + 1)], 1); });
        (void)simt::ballot(true);
        if (lane < kLenClasses) P.lq_cnt[(int64_t)lane * nchunks + c] = s_hist[wave][lane];
        (void)simt::ballot(true);
    }
}
TKZ_KERNEL(256) void k_long_scatter(EncodeParams P) {
    if (tkz_attempt_failed(P)) return;
    TKZ_SHARED int s_hist[4][kLenClasses];
    const int lane = simt::lane(), wave = simt::wave();
    const int64_t nchunks = (P.nsub + 63) / 64;
    for (int64_t c = simt::bid() * 4 + wave; c < nchunks; c += simt::nblocks() * 4) {
        if (lane < kLenClasses) s_hist[wave][lane] = 0;
        (void)simt::ballot(true);
        // the giant piece of a sub-tile (its last piece): merged by k_giant_merge before this kernel, its token count joins the sub-tile's here
        { const int64_t t = c * 64 + lane; if (t < P.nsub && (P.heavy_flag[t] & 2u)) { const int g = P.giant_cnt[t]; if (g > 1) simt::atomic_add(&P.tile_count[t], g - 1); } }   // (< 0: no pool, the call is retried)
        tkz_long_walk(P, c, P.lane_piece, [&](int64_t t, int j, uint32_t ent) {
            const int cl = tkz_len_class((int)((ent >> kMrLenShift) & 1023u) + 1);
            const int64_t at = P.lq_base[(int64_t)cl * nchunks + c] + simt::atomic_add(&s_hist[wave][cl], 1);
            if (at < P.lq_cap) P.lq[at] = ((uint64_t)t << 30) | ((uint64_t)j << 20) | (uint64_t)(ent & 0xFFFFFu);      // (ent: relpos | (len - 1) << 10)
        });
        (void)simt::ballot(true);
    }
}
template <bool COMPACT>
TKZ_KERNEL_OCC(64, 4) void k_merge_long_q(TkzTables T, EncodeParams P) {
    if (tkz_attempt_failed(P)) return;
    // LDS: the arena and the byte ids, 10 KB together -- sixteen wavefronts a CU (the chunk form's 12.4 KB: thirteen) --; 2,304 dwords are 64 spans of the
    // nine quads a piece of up to 28 bytes takes (52 of the eleven of 29..32 bytes)
    TKZ_SHARED uint4 s_lds[(kQArenaDwords + 256) / 4];
    LongLds LD;
    LD.arena = reinterpret_cast<uint32_t*>(s_lds); LD.arena_dwords = kQArenaDwords; LD.brank = reinterpret_cast<int32_t*>(s_lds) + kQArenaDwords;
    LD.pre = nullptr; LD.cls = nullptr; LD.ord = nullptr;
    tkz_long_brank_init(T, LD.brank);
    const int lane = simt::lane();
    int err = 0;
    LongProf PF;
    tkz_long_prof_begin(P, PF);
    const int64_t total = *P.lq_total < P.lq_cap ? *P.lq_total : P.lq_cap;
    // Ranges: kLqRange entries of the classes the fast batches take (up to kFastPiece bytes: four or five batches of one class), kLqRangeLong of the longer
    // ones (a lane takes ~n^2 steps for those and a batch holds ~15 of them: in ranges of 256 real text's 100..128-byte pieces kept a few wavefronts for
    // 3.5 ms).  From the END of the queue -- the longest classes first --, so that what runs last is short.
    const int64_t nchunks = (P.nsub + 63) / 64;
    int64_t nfast = P.lq_base[(int64_t)tkz_len_class(kFastPiece + 1) * nchunks];
    if (nfast > total) nfast = total;
    // (a SHORT queue -- real text: half a million long misses in 268 MB -- is dealt out in smaller ranges, down to one batch of 64: with 256 a range there
    //  are fewer ranges than wavefronts and the kernel lasts as long as one wavefront's four or five batches one after the other)
    int64_t rfast = kLqRange;
    while (rfast > 64 && (nfast + rfast - 1) / rfast < simt::nblocks()) rfast >>= 1;
    const int64_t nrf = (nfast + rfast - 1) / rfast, nrl = (total - nfast + kLqRangeLong - 1) / kLqRangeLong;
    auto range_of = [&](int64_t r, int64_t* lo, int64_t* hi) {
        if (r >= nrf) { *lo = nfast + (r - nrf) * kLqRangeLong; *hi = *lo + kLqRangeLong < total ? *lo + kLqRangeLong : total; }
        else { *lo = r * rfast; *hi = *lo + rfast < nfast ? *lo + rfast : nfast; }
    };
    auto entry_of = [&](int64_t pos, int64_t hi) -> uint64_t { return pos < hi ? P.lq[pos] : 0ull; };
    int64_t rg = nrf + nrl - 1 - simt::bid();
    int64_t lo = 0, hi = 0;
    if (rg >= 0) range_of(rg, &lo, &hi);
    uint64_t ent = rg >= 0 ? entry_of(lo + lane, hi) : 0ull;        // this batch's entry; the next batch's is requested as soon as this one's size is known
    while (rg >= 0) {
#ifdef TKZ_DEVPROF
        if (PF.on) { ++PF.units; PF.t0 = simt::clock(); }
#endif
        int64_t nlo = 0, nhi = 0;
        const int64_t nrg = rg - simt::nblocks();
        if (nrg >= 0) range_of(nrg, &nlo, &nhi);
        for (int64_t at = lo; at < hi;) {
            const bool valid = at + lane < hi;
            const int64_t sub = valid ? (int64_t)(ent >> 30) : 0;
            const int j = valid ? (int)((ent >> 20) & 1023u) : 0, len = valid ? (int)((ent >> 10) & 1023u) + 1 : 1, rel = valid ? (int)(ent & 1023u) : 0;
            uint64_t ent_next = 0;
            TKZ_PF_MARK(0);
            const int limit = tkz_long_batch<COMPACT>(T, P, LD, valid, sub, j, rel, len, P.lane_piece, err, PF, [&](int n) {
                const int64_t nx = at + n;                                  // the next batch: the rest of this range, else the wavefront's next range
                ent_next = nx < hi ? entry_of(nx + lane, hi) : (nrg >= 0 ? entry_of(nlo + lane, nhi) : 0ull);
            });
            at += limit;
            ent = ent_next;
        }
        rg = nrg; lo = nlo; hi = nhi;
    }
    if (err) simt::atomic_or((unsigned*)&P.counters[0], (unsigned)err);
    tkz_long_prof_end(P, PF);
}

// The missed pieces of kLanePiece + 1 .. kArenaPiece bytes: ONE WAVEFRONT per piece, with the giant pieces' merger (tkz_bpe_long_tail: batches of proposals with
// local bounds + rounds for chains of equal pairs -- its workgroup is this kernel's single wavefront, 32 slots a lane).  A lane of k_merge_long takes ~n^2 steps
// for a piece of n bytes and the kernel lasts as long as its slowest lane: one 1000-byte run of one letter held it for 3.4 ms, 40 times what the rest of a
// 1 GB batch needed; the wavefront takes ~30 batches whatever the length.  (Below kLanePiece the lanes win: 64 pieces a wavefront instead of one.)
// k_merge_long leaves such an entry as k_probe wrote it; k_probe has flagged the sub-tile (bit 2 of heavy_flag), k_list_stats queues the flagged sub-tiles' entries.
constexpr int kCoopScratch = (4 * kTailSubs + 8) * 64 + 16 + 16;
constexpr int kCoopLdsBytes = 2 * 4 * kArenaPiece + 4 * (kArenaPiece / 32) + kCoopScratch;
#ifdef TKZ_HOSTEMU
constexpr int kCoopGrid = 4;          // (the CPU emulator pays for every idle workgroup)
#else
constexpr int kCoopGrid = 2048;
#endif
constexpr int kCoopLdsQuads = (kCoopLdsBytes + 15) / 16;
// one wavefront, number `bid` of `nblocks`, over the queue (the body of k_merge_coop; k_merge_latency runs it beside the other two merge stages)
TKZ_DEV void tkz_merge_coop_queue(const TkzTables& T, const EncodeParams& P, uint4* s_lds, unsigned long long bid, unsigned long long nblocks) {
    int32_t* ids = reinterpret_cast<int32_t*>(s_lds);
    int32_t* pr = ids + kArenaPiece;
    uint32_t* alive = reinterpret_cast<uint32_t*>(pr + kArenaPiece);
    uint8_t* scratch = reinterpret_cast<uint8_t*>(alive + kArenaPiece / 32);
    const int lane = simt::lane();
    int err = 0;
    // The pieces wait in a queue (k_list_stats: sub-tile << 10 | index in its long list); a wavefront takes the next one off a ticket counter until
    // there is none.  (Until round 5 a wavefront owned chunks of 64 sub-tiles and merged the pieces of a chunk one after the other: a file of CJK prose --
    // 64 KiB of nothing but such pieces -- kept ONE wavefront busy for milliseconds.)
    // (a workgroup's FIRST piece is the one with its own number -- no atomic at all when the queue is shorter than the grid, in particular when it is
    //  empty: two thousand device-scope atomics on one address are not free --, the later ones come off the ticket counter)
    const unsigned long long count = *P.coop_count < (unsigned long long)P.coop_cap ? *P.coop_count : (unsigned long long)P.coop_cap;
    bool first = true;
    for (;;) {
        unsigned long long tk = bid;
        if (!first) {
            if (lane == 0) tk = nblocks + simt::atomic_add64(P.coop_ticket, 1ull);
            tk = ((unsigned long long)simt::shflu((uint32_t)(tk >> 32), 0) << 32) | simt::shflu((uint32_t)tk, 0);
        }
        first = false;
        if (tk >= count) break;
        const uint64_t qe = P.coop_q[tk];
        const int64_t sub = (int64_t)(qe >> 10);
        const int jj = (int)(qe & 1023u);
        const uint32_t ee = P.mlist[sub * (int64_t)P.mcap + (P.mcap - 1 - jj)];
        if (ee & kMrDone) continue;                             // (cannot happen: an entry is queued once)
        const int rel = (int)(ee & 1023u), n = (int)((ee >> kMrLenShift) & 1023u) + 1;
        const int64_t abs = sub * kSub + rel;
        const uint8_t* gb = P.bytes + abs;
        for (int k = lane; k < n; k += 64) {
            const uint32_t b = gb[k];
            ids[k] = T.byte_rank[b];
            pr[k] = (k + 1 < n) ? T.bytepair_rank[(b << 8) | gb[k + 1]] : TKZ_RANK_NONE;
        }
        simt::sync();
        tkz_bpe_long_tail<true>(T, n, ids, pr, alive, scratch, nullptr);
        const int cnt = tkz_bpe_long_tail_emit<true>(n, ids, pr, alive, P.tmp + abs, &err);
        if (lane == 0) {
            P.mlist[sub * (int64_t)P.mcap + (P.mcap - 1 - jj)] = tkz_result_entry(false, cnt, rel);      // (the tokens are in tmp at the piece's position)
            if (cnt > 1) simt::atomic_add(&P.tile_count[sub], cnt - 1);
        }
        simt::sync();
    }
    if (err) simt::atomic_or((unsigned*)&P.counters[0], (unsigned)err);
}
TKZ_KERNEL(64) void k_merge_coop(TkzTables T, EncodeParams P) {
    if (tkz_attempt_failed(P)) return;
    TKZ_SHARED uint4 s_lds[kCoopLdsQuads];
    tkz_merge_coop_queue(T, P, s_lds, (unsigned long long)simt::bid(), (unsigned long long)simt::nblocks());
}

// A SMALL batch (TKZ_OPT_LATENCY_BYTES) waits for the slowest wavefront of every kernel and for every dispatch: its two large merge stages -- the short misses, the
// long ones in the chunk form -- touch different list entries and add their tokens to the sub-tiles' counts with atomics (EncodeParams::tc_atomic: k_probe has
// zeroed them), so they run as ONE launch: workgroups [0, nb_short) are k_merge_short's, block for block (four groups of 16 sub-tiles each, the same XCD order:
// the piece memo is shared through an XCD's L2 -- a wavefront a workgroup, spread over the eight XCDs, cut a 160 KB batch's memo hits from most lookups to 6 %),
// workgroups [nb_short, nb_short + nb_long) take the units of the long lists, a wavefront each.  A 1 MB call: k_merge_short 33 us + k_merge_long 45 us one after
// the other, each behind its own dispatch; 240 -> 210 us a call.
constexpr int kMergeLatWaveQuads = kMsLdsQuads > kLongLdsQuads ? kMsLdsQuads : kLongLdsQuads;
template <bool COMPACT>
TKZ_KERNEL_OCC(kMsThreads, 3) void k_merge_latency(TkzTables T, EncodeParams P, int nb_short, int nb_long) {
    if (tkz_attempt_failed(P)) return;
    TKZ_SHARED uint4 s_wave[kMsThreads / 64][kMergeLatWaveQuads];
    TKZ_SHARED uint16_t s_brank16[256];
    const int b = (int)simt::bid();
    if (b < nb_short) {                                     // (wave-uniform, block-uniform: the barrier below is reached by the whole workgroup or not at all)
        tkz_ms_brank_init(T, s_brank16);
        simt::sync();
        const int64_t grp = tkz_xcd_block(b, nb_short) * (kMsThreads / 64) + simt::wave();
        tkz_merge_short_group(T, P, grp, tkz_ms_lds(s_wave[simt::wave()], s_brank16));
    } else {
        const LongLds LD = tkz_long_lds(s_wave[simt::wave()]);
        tkz_long_brank_init(T, LD.brank);
        tkz_merge_long_chunks<COMPACT, kLongPartsLatency, -1>(T, P, (int64_t)(b - nb_short) * (kMsThreads / 64) + simt::wave(), (int64_t)nb_long * (kMsThreads / 64), LD, P.lane_piece);
    }
}

// ids at their final position: count per record -> prefix -> the sub-tile's ids staged in LDS -> stored as whole 16-byte quads (one
// store instruction = 16 full lines; per-lane 4-byte stores at variable offsets wrote 1.8x the bytes); the token index (inside the
// sub-tile) of every marked piece
#ifndef TKZ_PLACE_OCC
#define TKZ_PLACE_OCC 7
#endif
// Answers (and quads) of a sub-tile's miss lists that k_place keeps in LDS: SLOTS = 64 (one per lane: the short list from slot 0 up, the long one from
// slot 63 down; a sub-tile of the bench corpus averages 14 short misses and one long one) or 128 (two per lane, the second half only for
// sub-tiles that keep more than 64).  The 128-slot form costs every sub-tile ~5 % (its instructions, its LDS) and saves a miss-heavy batch
// 40 % of the kernel (a vocabulary that has not seen the text: 75 misses per sub-tile, most of them above 64, which the 64-slot form hands
// to its general path): the host launches it when more than a fifth of the sub-tiles of the workspace's previous batch held more than 64
// entries (k_probe counts them on every 64th sub-tile; EncodeParams::place128).
constexpr int kPlacePer = 4;                               // consecutive sub-tiles per wavefront of k_place
constexpr int kPlaceBig = 8;                               // the general path: token runs longer than this are copied by the whole wavefront, not staged
#ifndef TKZ_PLACE_FAST_BIG
#define TKZ_PLACE_FAST_BIG 64
#endif
constexpr int kPlaceFastBig = TKZ_PLACE_FAST_BIG;                          // the fast path takes sub-tiles whose longest token run is at most this (a lane copies its piece's tokens into the stage)
constexpr int kStageMin = 64 * kPlaceBig + 16;             // staged ids: after a flush, the <= 64 x kPlaceBig ids of one batch of records + the alignment shift always fit
// ... and what k_place's wavefronts keep: the fast path stages the ids of 256 records at once and hands a chunk that does not fit to the general path (64 records at a
// time, four times the scans) -- text of two tokens a piece (source text under the gpt2 table: 1.75) did that for every fifth chunk with 528 ids of room
#ifndef TKZ_PLACE_STAGE
#define TKZ_PLACE_STAGE 784
#endif
constexpr int kStageBatch = TKZ_PLACE_STAGE;
static_assert(kStageBatch >= kStageMin && kStageBatch % 16 == 0, "whole quads, and room for one batch of the general path");
// LDS of one wavefront of k_place: the staged ids, the first answers of the sub-tile's short-miss list and of the long one, and the quads
// of those entries (the tokens of pieces of <= 4)
// ... the token position of every kept entry's piece (the fast path: the lane that owns the record tells the lane that owns the entry)
template <int SLOTS, int STAGE> constexpr int kPlaceLdsQuadsT = STAGE / 4 + SLOTS + SLOTS / 4 + 1 + SLOTS / 4;
constexpr int kPlaceLdsQuads = kPlaceLdsQuadsT<64, kStageMin>;       // (the single-launch kernel always uses the 64-slot form, with the smallest stage)
struct PlaceLds { int32_t* stage; uint4* quad; uint32_t* res; int32_t* pos; };
template <int SLOTS, int STAGE>
TKZ_DEV PlaceLds tkz_place_lds(uint4* wave_quads) {
    constexpr int kStage = STAGE;
    PlaceLds L;
    L.stage = reinterpret_cast<int32_t*>(wave_quads);
    L.quad = wave_quads + kStage / 4;
    L.res = reinterpret_cast<uint32_t*>(wave_quads + kStage / 4 + SLOTS);                       // SLOTS answers + slot SLOTS: "one token"
    L.pos = reinterpret_cast<int32_t*>(wave_quads + kStage / 4 + SLOTS + SLOTS / 4 + 1);
    return L;
}
// sub-tiles sub0 .. sub0 + kPlacePer - 1, by one wavefront
// PROMO: the tables hold promoted pieces (tkz_tables.h): a hit record may carry a promo code instead of a rank -- its count is in the record, its
// tokens are one 16-byte gather from P.promo.  The form without them is the kernel of every batch before the first promotion, instruction for instruction.
// The seven per-sub-tile arrays of scalars come as restrict parameters of their own: nothing in here stores to them, and a compiler that is told so reads
// them with scalar loads inside the loop too (a load behind the loop's stores is otherwise a vector load: ten vector registers a set, and a readfirstlane each).
template <int SLOTS, bool PROMO, int STAGE>
TKZ_DEV void tkz_place_subtiles_sc(const EncodeParams& P, int32_t* out, int64_t out_cap, int64_t sub0, const PlaceLds& LD,
                                   const int64_t* __restrict__ pbase, const int64_t* __restrict__ tile_base, const int64_t* __restrict__ docord_base, const int32_t* __restrict__ pcount,
                                   const uint32_t* __restrict__ mcount, const uint8_t* __restrict__ heavy_flag, const int32_t* __restrict__ giant_cnt) {
    constexpr int kPlaceSlots = SLOTS, kPlaceRes = SLOTS / 2, kStage = STAGE;
    const int lane = simt::lane();
    if (sub0 >= P.nsub) return;
    int32_t* stage = LD.stage;
    uint32_t* s_res = LD.res;
    uint4* s_quad = LD.quad;
    int32_t* s_pos = LD.pos;
    // what a wavefront needs to know about a sub-tile before it can ask for its records and answers: seven wave-uniform words
    struct Sc { int64_t pb, tb, ord0; int np; uint32_t mc, hf; int gc; };
    auto load_sc = [&](int64_t sub) -> Sc {
        Sc c;
        c.pb = pbase[sub]; c.tb = tile_base[sub]; c.ord0 = docord_base[sub]; c.np = pcount[sub]; c.mc = mcount[sub]; c.hf = heavy_flag[sub]; c.gc = giant_cnt[sub];
        return c;
    };
    // the lane's four records of a chunk of a sub-tile (records kk + 4 * lane .. + 3: one 16-byte load)
    auto load_recs = [&](int64_t pb_, int np_, int kk, uint32_t* r) {
        // (a scalar base and a 32-bit lane offset: no 64-bit address or comparison a lane)
        const int k0 = kk + 4 * lane;
        const int32_t* const recs = P.prank + pb_;
        const int64_t room64 = P.prank_cap - pb_;
        const int room = room64 < 0 ? 0 : room64 > (1 << 20) ? (1 << 20) : (int)room64;          // records of this sub-tile (at most 1,024) that the buffer holds
        r[0] = r[1] = r[2] = r[3] = 0u;
        if (k0 < np_) {
            if (k0 + 4 <= room) { const uint4 v = tkz_load16_nt(&recs[(uint32_t)k0]); r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w; }
            else for (int j = 0; j < 4; ++j) if (k0 + j < room) r[j] = (uint32_t)recs[(uint32_t)(k0 + j)];
        }
    };
    // which list entries of a sub-tile are kept in LDS, from its miss counts alone (all wave-uniform): slots 0 .. ks-1 hold the first ks entries
    // of the short list, slots top .. top-kl+1 the first kl of the long one
    static_assert(SLOTS == 64 || SLOTS == 128, "one or two kept entries per lane: slots lane and lane + 64");
    struct Kept { int ks, kl, top; bool two, lists_ok; };
    auto kept_of = [&](uint32_t mc_) -> Kept {
        const int ns_ = (int)(mc_ & 0xFFFFu), nl_ = (int)(mc_ >> 16);
        Kept k;
        k.lists_ok = ns_ + nl_ <= P.mcap;                     // (cut lists: the batch is redone, nothing of this pass is used)
        k.kl = ns_ + nl_ <= kPlaceSlots ? nl_ : (nl_ < kPlaceRes ? nl_ : kPlaceRes);
        k.ks = ns_ < kPlaceSlots - k.kl ? ns_ : kPlaceSlots - k.kl;
        k.two = SLOTS == 128 && k.ks + k.kl > 64;             // (wave-uniform: the second slot of every lane is in use; never with 64 slots)
        k.top = k.two ? kPlaceSlots - 1 : 63;                 // entry e of the long list is kept in slot top - e
        return k;
    };
    // the answer and the quad of the entry kept in slot lane + 64 * h of sub-tile sub_ (zero where the slot keeps none)
    auto load_ans = [&](int64_t sub_, const Kept& k, int h, uint32_t& a, uint4& qd) {
        a = 0u; qd.x = qd.y = qd.z = qd.w = 0;
        const int slot = lane + 64 * h;
        const bool shortside = slot < k.ks;
        const int e = shortside ? slot : k.top - slot;
        const bool want = k.lists_ok && (shortside || e < k.kl);
        const uint32_t at = (uint32_t)((shortside ? e : P.mcap - 1 - e) & (kMissCapMax - 1));
        const uint32_t* const ml_ = P.mlist + sub_ * (int64_t)P.mcap;
        const uint4* const mqd_ = P.mquad + sub_ * (int64_t)P.mcap;
        if (want) { a = tkz_load_nt(&ml_[at]); qd = tkz_load16_nt(&mqd_[at]); }
    };
    // A wavefront places kPlacePer consecutive sub-tiles, one after the other.  A sub-tile's answers and its first 256 records are requested together at its top,
    // ahead of the LDS fill (one round trip), and then the seven scalars of the sub-tile behind it, which arrive while this one is placed.  (Requesting records
    // and answers a whole sub-tile ahead, in registers, was built and measured and is not here: profiles/place_pipeline.)
    Sc nxt = load_sc(sub0);
#pragma unroll 1
    for (int it = 0; it < kPlacePer && sub0 + it < P.nsub; ++it) {
    const int64_t sub = sub0 + it;
    // (k_small's scalars come through vector loads -- they were stored by this very kernel --: told that they are uniform, they leave the vector registers here)
    Sc cur;
    cur.pb = (int64_t)simt::uniform64((uint64_t)nxt.pb); cur.tb = (int64_t)simt::uniform64((uint64_t)nxt.tb); cur.ord0 = (int64_t)simt::uniform64((uint64_t)nxt.ord0);
    cur.np = simt::first_lane(nxt.np); cur.mc = (uint32_t)simt::first_lane((int)nxt.mc); cur.hf = (uint32_t)simt::first_lane((int)nxt.hf); cur.gc = simt::first_lane(nxt.gc);
    const Kept kp = kept_of(cur.mc);
    uint32_t a[2] = {0u, 0u}, r_cur[4];
    uint4 qd[2];
    load_ans(sub, kp, 0, a[0], qd[0]);
    load_recs(cur.pb, cur.np, 0, r_cur);
    if (it + 1 < kPlacePer && sub + 1 < P.nsub) nxt = load_sc(sub + 1);
    const int64_t pb = cur.pb, tb = cur.tb, base = sub * kSub, ord0 = cur.ord0;
    const int np = cur.np;
    const uint32_t mc = cur.mc;
    const int ns = (int)(mc & 0xFFFFu), nl = (int)(mc >> 16);
    const uint32_t* const ml = P.mlist + sub * (int64_t)P.mcap;
    const uint4* const mqd = P.mquad + sub * (int64_t)P.mcap;
    const int32_t* const dense = P.dense + (sub / kGroup) * kDenseCap;
    const bool has_giant = (cur.hf & 2u) != 0;
    int gcnt = has_giant ? cur.gc : 0;
    if (gcnt < 0) gcnt = 0;
    const bool lists_ok = kp.lists_ok;
    const int kl = kp.kl, ks = kp.ks, top = kp.top;
    const bool two = kp.two;
    bool fast_ok;
    {
        // lane l fills slot l and -- only when more than 64 entries are kept (top = 127 then, else 63) -- slot l + 64, whose entry is loaded here
        qd[1].x = qd[1].y = qd[1].z = qd[1].w = 0;
        if (two) load_ans(sub, kp, 1, a[1], qd[1]);
        const bool big = tkz_result_cnt(a[0]) > kPlaceFastBig || tkz_result_cnt(a[1]) > kPlaceFastBig;
        (void)simt::ballot(true);                                // (the sub-tile before this one is done with them)
        s_res[lane] = a[0]; s_quad[lane] = qd[0]; s_pos[lane] = -1;
        if constexpr (SLOTS == 128) { s_res[lane + 64] = a[1]; s_quad[lane + 64] = qd[1]; s_pos[lane + 64] = -1; }
        if (lane == 0) s_res[kPlaceSlots] = tkz_result_inline(1);
        // The fast path (below) takes a sub-tile whose lists are wholly in LDS (kPlaceSlots entries together) and hold no token run longer
        // than kPlaceFastBig, and that has no giant piece: nearly all of them.
        fast_ok = lists_ok && !has_giant && ns + nl <= kPlaceSlots && !simt::ballot(big);
    }
    (void)simt::ballot(true);
    // the answer a merge kernel left for a missed piece (its list entry): how many tokens, and where they wait
    auto answer = [&](uint32_t rec) -> uint32_t {
        if (rec & kPrGiant) return tkz_result_entry(false, 1, (int)(rec & 1023u));     // (count: gcnt, see below; the tokens wait in tmp at the piece's position)
        const int idx = (int)(rec & 1023u);
        const bool lg = (rec & kPrLong) != 0;
        if (!lists_ok) return tkz_result_inline(1);
        return (lg ? idx < kl : idx < ks) ? s_res[lg ? top - idx : idx] : ml[lg ? P.mcap - 1 - idx : idx];
    };
    // ... its tokens: INLINE (<= 4 tokens, nearly every missed piece: in the entry's quad, which for the first entries of both lists is
    // already in LDS), else in the group's dense region or in tmp
    auto inline_quad = [&](uint32_t rec) -> uint4 {
        const int idx = (int)(rec & 1023u);
        const bool lg = (rec & kPrLong) != 0;
        if (!lists_ok) { uint4 z; z.x = z.y = z.z = z.w = 0; return z; }
        return (lg ? idx < kl : idx < ks) ? s_quad[lg ? top - idx : idx] : tkz_load16(&mqd[lg ? P.mcap - 1 - idx : idx]);
    };
    auto token_src = [&](uint32_t res) -> const int32_t* { return (res & kMrDense) ? dense + tkz_result_off(res) : P.tmp + base + tkz_result_off(res); };
    // stage[i] holds the id of token sbase + i of the sub-tile; sbase is chosen so that stage[0] sits on a 16-byte boundary of `out`
    const uintptr_t out_addr = reinterpret_cast<uintptr_t>(out);
    auto quad_base = [&](int tok) -> int { return tok - (int)(((out_addr >> 2) + (uintptr_t)(tb + tok)) & 3u); };
    int running = 0, marks = 0, flushed = 0, sbase = quad_base(0);
    auto flush = [&](int upto) {                             // stores tokens [flushed, upto) of the sub-tile
        (void)simt::ballot(true);
        const int lo = flushed - sbase, hi = upto - sbase;
        // (wave-uniform, and said to be: a lane adds a 32-bit offset to a scalar base -- left to itself the compiler keeps out + 16 * lane in two vector registers across the loop)
        int32_t* const obase = reinterpret_cast<int32_t*>(simt::uniform64(reinterpret_cast<uintptr_t>(out + tb + sbase)));
        const int64_t oroom64 = out_cap - tb - sbase;
        const int oroom = oroom64 < 0 ? 0 : oroom64 > (1 << 20) ? (1 << 20) : (int)oroom64;      // ids of the stage (a few thousand at most) that `out` has room for
        for (int q4 = lane; 4 * q4 < hi; q4 += 64) {
            const int i0 = 4 * q4;
            if (i0 + 4 <= lo) continue;
            const uint4 v = reinterpret_cast<const uint4*>(stage)[q4];
            int32_t* dst = obase + (uint32_t)i0;
            if (i0 >= lo && i0 + 4 <= hi && i0 + 4 <= oroom) tkz_store16_nt(dst, v);
            else {
                const int32_t w[4] = {(int32_t)v.x, (int32_t)v.y, (int32_t)v.z, (int32_t)v.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) if (i0 + i >= lo && i0 + i < hi && i0 + i < oroom) dst[i] = w[i];
            }
        }
        (void)simt::ballot(true);
        flushed = upto; sbase = quad_base(upto);
    };
    // ---- the fast path: FOUR CONSECUTIVE records per lane (one 16-byte load), so that 256 records cost one wave scan, one pass over the
    // marks and one pass over the missed pieces instead of four of each -- k_place runs at the VALU issue limit, and what it issues is
    // mostly per-batch overhead.  A record's token count comes from LDS without a branch (a hit reads the "one token" slot); the
    // tokens of a missed piece are written by the lane that OWNS its list entry's slot (slot e: entry e of the short list, slot top - e: entry e
    // of the long one; lane l owns slots l and l + 64): the lane that holds the record only tells it the position. ----
    const int64_t room64 = P.prank_cap - pb;
    const int nrec = room64 < np ? (room64 < 0 ? 0 : (int)room64) : np;       // the sub-tile's records that the buffer holds: all of them, unless the attempt is one to be thrown away
    int32_t* const doc_tok = P.doc_tok + ord0;
    int32_t* const otile = reinterpret_cast<int32_t*>(simt::uniform64(reinterpret_cast<uintptr_t>(out + tb)));      // (the general path's direct stores: a scalar base too)
    auto place_fast = [&](int kk) -> bool {
        const int k0 = kk + 4 * lane;
        uint32_t r[4] = {r_cur[0], r_cur[1], r_cur[2], r_cur[3]};     // the first chunk's were requested with the answers
        if (kk) load_recs(pb, np, kk, r);
        int c[4], idx[4];
        bool ok[4], ms[4], pm[4];
        uint4 pq0;                                               // the token quad of the lane's FIRST promoted record
        int pj = -1, pdst = 0, pcnt = 0;
        int t = 0, mk = 0;
        if constexpr (PROMO) {
#pragma unroll
            for (int j = 3; j >= 0; --j) { pm[j] = k0 + j < nrec && !(r[j] & kPrMiss) && (r[j] & kPromoFlag); if (pm[j]) pj = j; }
            // One promoted piece in a hundred: a lane's four records hold one at most, nearly always.  ITS quad is requested here, ahead of the scan, and its
            // tokens are staged after the missed pieces' below -- the round trip to the promo array overlaps both (four registers across them; all four
            // records' quads, requested after the scan and waited for at once, were a dependent round trip per 256 records: 1.0 of k_place's 4.75 ms).  A
            // second promoted record of the same lane fetches its quad on the spot.
            pq0 = tkz_load16(&P.promo[pj >= 0 ? (r[pj >= 0 ? pj : 0] & kPromoIdxMask) : 0u]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ok[j] = k0 + j < nrec;
            ms[j] = ok[j] && (r[j] & kPrMiss);
            idx[j] = ((r[j] & kPrLong) ? top - (int)(r[j] & 1023u) : (int)(r[j] & 1023u)) & (kPlaceSlots - 1);     // the slot of the piece's list entry
            const uint32_t a = s_res[ms[j] ? idx[j] : kPlaceSlots];
            c[j] = ok[j] ? tkz_result_cnt(a) : 0;
            if constexpr (PROMO) { if (pm[j]) c[j] = (int)((r[j] >> kPromoCntShift) & 3u) + 1; }
            t += c[j];
            mk += (ok[j] && (r[j] & kPrMark)) ? 1 : 0;
        }
        int both;
        const int pre = tkz_wave_scan_sum(t | (mk << 20), &both);
        const int tot = both & 0xFFFFF, mtot = both >> 20;
        if (running + tot - sbase > kStage) {
            if (flushed < running) flush(running);
            if (running + tot - sbase > kStage) return false;        // (more than two tokens a record: the general path, 64 records at a time)
        }
        int pos = running + (pre & 0xFFFFF), mi = marks + (pre >> 20);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (ok[j] && (r[j] & kPrMark)) doc_tok[(uint32_t)mi++] = pos;
            if (ms[j]) s_pos[idx[j]] = pos;
            else if (PROMO && pm[j]) {
                if (j == pj) { pdst = pos - sbase; pcnt = c[j]; }
                else {                                           // (rare: a second promoted record in this lane's four)
                    const uint4 q = tkz_load16(&P.promo[r[j] & kPromoIdxMask]);
                    int32_t* dst = stage + (pos - sbase);
                    dst[0] = (int32_t)q.x;
                    if (c[j] > 1) dst[1] = (int32_t)q.y;
                    if (c[j] > 2) dst[2] = (int32_t)q.z;
                    if (c[j] > 3) dst[3] = (int32_t)q.w;
                }
            }
            else if (ok[j]) stage[pos - sbase] = (int32_t)(r[j] & kPrRankMask);
            pos += c[j];
        }
        (void)simt::ballot(true);
        // the missed pieces of this chunk, by the lanes that own their entries (slot lane, and slot lane + 64 when that half is in use)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && !two) break;
            const int slot = lane + 64 * h;
            const int p = s_pos[slot];
            if (p >= 0) {                                        // (set once per entry, by the lane that holds its record)
                const uint32_t ans = s_res[slot];
                const int cnt = tkz_result_cnt(ans);
                int32_t* dst = stage + (p - sbase);
                if (ans & kMrInline) {
                    const uint4 q = s_quad[slot];
                    dst[0] = (int32_t)q.x;
                    if (cnt > 1) dst[1] = (int32_t)q.y;
                    if (cnt > 2) dst[2] = (int32_t)q.z;
                    if (cnt > 3) dst[3] = (int32_t)q.w;
                } else {
                    const int32_t* src = token_src(ans);
                    for (int i = 0; i < cnt; ++i) dst[i] = src[i];
                }
                s_pos[slot] = -1;
            }
        }
        if constexpr (PROMO) {
            if (pcnt) {
                int32_t* dst = stage + pdst;
                dst[0] = (int32_t)pq0.x;
                if (pcnt > 1) dst[1] = (int32_t)pq0.y;
                if (pcnt > 2) dst[2] = (int32_t)pq0.z;
                if (pcnt > 3) dst[3] = (int32_t)pq0.w;
            }
        }
        running += tot; marks += mtot;
        return true;
    };
#pragma unroll 1
    for (int kk = 0; kk < np; kk += 256) {                     // four record loads in flight per lane
      if (fast_ok && place_fast(kk)) continue;
      // ---- the general path (giant pieces, long token runs, lists longer than LDS keeps): 64 records at a time ----
#pragma unroll 1
      for (int j = 0; j < 4; ++j) {
        const int k0 = kk + 64 * j;
        if (k0 >= np) break;
        const int k = k0 + lane;
        const bool valid = k < nrec;
        const uint32_t rec = valid ? (uint32_t)tkz_load_nt(&(P.prank + pb)[(uint32_t)k]) : 0u;
        const uint32_t res = (rec & kPrMiss) ? answer(rec) : 0u;           // the merge kernels' answer for a missed piece
        const bool miss = (rec & kPrMiss) != 0;
        const bool promoted = PROMO && valid && !miss && (rec & kPromoFlag);
        uint4 pquad; pquad.x = pquad.y = pquad.z = pquad.w = 0;
        if constexpr (PROMO) { if (promoted) pquad = tkz_load16(&P.promo[rec & kPromoIdxMask]); }
        const int cnt = !valid ? 0 : !miss ? (promoted ? (int)((rec >> kPromoCntShift) & 3u) + 1 : 1) : (rec & kPrGiant) ? gcnt : tkz_result_cnt(res);
        int tot;
        const int pos = running + tkz_wave_scan_sum(cnt, &tot);
        const uint64_t mm = simt::ballot(valid && (rec & kPrMark));
        if (valid && (rec & kPrMark)) doc_tok[(uint32_t)(marks + tkz_popc64(mm & tkz_lowmask(lane)))] = pos;
        const uint64_t big = simt::ballot(valid && miss && cnt > kPlaceBig);
        if (!big) {
            if (running + tot - sbase > kStage) flush(running);
            if (valid) {
                int32_t* dst = stage + (pos - sbase);
                if (promoted) {
                    dst[0] = (int32_t)pquad.x;
                    if (cnt > 1) dst[1] = (int32_t)pquad.y;
                    if (cnt > 2) dst[2] = (int32_t)pquad.z;
                    if (cnt > 3) dst[3] = (int32_t)pquad.w;
                }
                else if (!miss) dst[0] = (int32_t)(rec & kPrRankMask);
                else if (res & kMrInline) {
                    const uint4 q = inline_quad(rec);
                    dst[0] = (int32_t)q.x;
                    if (cnt > 1) dst[1] = (int32_t)q.y;
                    if (cnt > 2) dst[2] = (int32_t)q.z;
                    if (cnt > 3) dst[3] = (int32_t)q.w;
                } else {
                    const int32_t* src = token_src(res);
                    for (int i = 0; i < cnt; ++i) dst[i] = src[i];
                }
            }
        } else {
            // a long token run (a merged piece of many bytes, a giant piece) in this batch of 64 records: what is staged goes out, then
            // this batch's ids go straight to their positions, the long runs copied by the whole wavefront, one after the other
            flush(running);
            const int32_t* src = (miss && !(res & kMrInline)) ? token_src(res) : nullptr;
            if (valid) {
                int32_t* dst = otile + (uint32_t)pos;
                if (promoted) {
                    const int32_t w[4] = {(int32_t)pquad.x, (int32_t)pquad.y, (int32_t)pquad.z, (int32_t)pquad.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (i < cnt && tb + pos + i < out_cap) dst[i] = w[i];
                }
                else if (!miss) { if (tb + pos < out_cap) tkz_store_nt(&dst[0], (int32_t)(rec & kPrRankMask)); }
                else if (res & kMrInline) {
                    const uint4 q = inline_quad(rec);
                    const int32_t w[4] = {(int32_t)q.x, (int32_t)q.y, (int32_t)q.z, (int32_t)q.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (i < cnt && tb + pos + i < out_cap) dst[i] = w[i];
                } else if (cnt <= kPlaceBig) {
                    for (int i = 0; i < cnt; ++i) if (tb + pos + i < out_cap) dst[i] = src[i];
                }
            }
            for (uint64_t bg = big; bg; bg &= bg - 1) {
                const int src_lane = tkz_ctz64(bg);
                const int c = simt::shfl(cnt, src_lane), p0 = simt::shfl(pos, src_lane);
                const uint32_t lo32 = simt::shflu((uint32_t)(reinterpret_cast<uintptr_t>(src)), src_lane), hi32 = simt::shflu((uint32_t)(reinterpret_cast<uintptr_t>(src) >> 32), src_lane);
                const int32_t* bsrc = reinterpret_cast<const int32_t*>(((uintptr_t)hi32 << 32) | lo32);
                int32_t* dst = otile + (uint32_t)p0;
                for (int i = lane; i < c; i += 64) if (tb + p0 + i < out_cap) dst[i] = bsrc[i];
            }
            flushed = running + tot; sbase = quad_base(flushed);
        }
        running += tot;
        marks += tkz_popc64(mm);
      }
    }
    if (flushed < running) flush(running);
    }
}
template <int SLOTS, bool PROMO, int STAGE>
TKZ_DEV void tkz_place_subtiles(const EncodeParams& P, const int64_t* tile_base, int32_t* out, int64_t out_cap, int64_t sub0, const PlaceLds& LD) {
    tkz_place_subtiles_sc<SLOTS, PROMO, STAGE>(P, out, out_cap, sub0, LD, P.pbase, tile_base, P.docord_base, P.pcount, P.mcount, P.heavy_flag, P.giant_cnt);
}
// (the 128-slot form's LDS, 24.9 KB a workgroup, admits six workgroups a CU: its bound says so)
template <int SLOTS, bool PROMO>
TKZ_KERNEL_OCC(256, SLOTS == 128 && TKZ_PLACE_OCC > 6 ? 6 : TKZ_PLACE_OCC) void k_place(EncodeParams P, const int64_t* tile_base, int32_t* out, int64_t out_cap) {
    if (tkz_attempt_failed(P)) return;
    TKZ_SHARED uint4 s_wave[kThreads / 64][kPlaceLdsQuadsT<SLOTS, kStageBatch>];
    const int64_t sub0 = (tkz_xcd_block(simt::bid(), simt::nblocks()) * (kThreads / 64) + simt::wave()) * kPlacePer;
    tkz_place_subtiles<SLOTS, PROMO, kStageBatch>(P, tile_base, out, out_cap, sub0, tkz_place_lds<SLOTS, kStageBatch>(s_wave[simt::wave()]));
}

// k_tokcount: the count form of k_place (a count call, tkz_count_*: the ids are never wanted).  It fills P.doc_tok -- the token index inside its sub-tile of
// every marked piece -- exactly as k_place does and stores nothing else: no id stage, no flush, no `out`; no atomics and no fence.  k_place's mapping (tkz_xcd_block,
// kPlacePer consecutive sub-tiles a wavefront, the next sub-tile's scalars requested while this one is counted, four consecutive records a lane from one 16-byte
// load), with two short cuts the ids do not allow:
//   * a sub-tile without a mark (dcount[sub] == 0: k_doccount2) is skipped for the price of its scalar loads -- on documents longer than a sub-tile, nearly all;
//   * a sub-tile with marks is walked until its last mark is written (marks == dcount[sub], wave-uniform): the records behind it are never loaded.
// The token count of a record is read as k_place reads it -- a hit 1, a promoted piece from its record bits, a missed piece tkz_result_cnt of its list entry, a
// giant piece giant_cnt[sub] -- and nothing but the count: mquad, dense, tmp and promo are never read.  LDS: one count word per list entry, kCountSlots entries in
// ONE form (the short list from slot 0 up, the long one from the top down; entries beyond them are read from the list in memory, as on k_place's general path), and
// slot kCountSlots: "one token".  One wave scan of tokens | marks << 20 per 256 records; a chunk in which a lane's four records stand for more than kCountLaneMax
// tokens (a giant piece, a long merged one: 64 lanes of at most that fit 20 bits) is taken 64 records at a time with a scan of the tokens alone.
// With cut lists (ns + nl > mcap) the attempt is redone and nothing of this pass is used: every missed piece counts 1 then, and nothing is read through the lists.
constexpr int kCountSlots = 128, kCountLaneMax = (1 << 20) / 64 - 1;
#ifndef TKZ_TOKCOUNT_OCC
#define TKZ_TOKCOUNT_OCC 8
#endif
TKZ_KERNEL_OCC(256, TKZ_TOKCOUNT_OCC) void k_tokcount(EncodeParams P, const int32_t* dcount) {
    if (tkz_attempt_failed(P)) return;
    TKZ_SHARED int32_t s_wave[kThreads / 64][kCountSlots + 4];
    const int lane = simt::lane();
    int32_t* const s_cnt = s_wave[simt::wave()];
    const int64_t sub0 = (tkz_xcd_block(simt::bid(), simt::nblocks()) * (kThreads / 64) + simt::wave()) * kPlacePer;
    if (sub0 >= P.nsub) return;
    const bool promo = P.promo != nullptr;                 // (a hit record may carry a promo code instead of a rank: tkz_tables.h)
    struct Sc { int64_t pb, ord0; int np, dc; uint32_t mc, hf; int gc; };
    auto load_sc = [&](int64_t sub) -> Sc {
        Sc c;
        c.dc = dcount[sub]; c.pb = P.pbase[sub]; c.ord0 = P.docord_base[sub]; c.np = P.pcount[sub]; c.mc = P.mcount[sub]; c.hf = P.heavy_flag[sub]; c.gc = P.giant_cnt[sub];
        return c;
    };
    Sc nxt = load_sc(sub0);
#pragma unroll 1
    for (int it = 0; it < kPlacePer && sub0 + it < P.nsub; ++it) {
        const int64_t sub = sub0 + it;
        const Sc cur = nxt;
        if (it + 1 < kPlacePer && sub + 1 < P.nsub) nxt = load_sc(sub + 1);
        const int dc = cur.dc;
        if (dc <= 0) continue;                               // (wave-uniform) no document starts here: nobody asks for a position inside this sub-tile
        const int64_t pb = cur.pb, ord0 = cur.ord0;
        const int np = cur.np;
        const int ns = (int)(cur.mc & 0xFFFFu), nl = (int)(cur.mc >> 16);
        const uint32_t* const ml = P.mlist + sub * (int64_t)P.mcap;
        const bool has_giant = (cur.hf & 2u) != 0;
        int gcnt = has_giant ? cur.gc : 0;
        if (gcnt < 0) gcnt = 0;
        const bool lists_ok = ns + nl <= P.mcap;
        // slot s holds the count of entry s of the short list (s < ks) or of entry top - s of the long one (s > top - kl); lane l loads slot l and -- only when
        // more than 64 entries are kept -- slot l + 64
        const int kl = ns + nl <= kCountSlots ? nl : (nl < kCountSlots / 2 ? nl : kCountSlots / 2), ks = ns < kCountSlots - kl ? ns : kCountSlots - kl;
        const bool two = ks + kl > 64;
        const int top = two ? kCountSlots - 1 : 63;
        {
            int a[2] = {1, 1};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 1 && !two) break;
                const int slot = lane + 64 * h;
                const bool shortside = slot < ks;
                const int e = shortside ? slot : top - slot;
                if (lists_ok && (shortside || e < kl)) a[h] = tkz_result_cnt(tkz_load_nt(&ml[shortside ? e : P.mcap - 1 - e]));
            }
            (void)simt::ballot(true);                            // (the sub-tile before this one is done with them)
            s_cnt[lane] = a[0]; s_cnt[lane + 64] = a[1];
            if (lane == 0) s_cnt[kCountSlots] = 1;
        }
        (void)simt::ballot(true);
        const bool all_kept = lists_ok && !has_giant && ns + nl <= kCountSlots;      // every missed piece's count is in LDS: nearly every sub-tile
        // the token count of a missed piece wherever its answer is
        auto miss_count = [&](uint32_t rec) -> int {
            if (rec & kPrGiant) return gcnt;
            if (!lists_ok) return 1;
            const int idx = (int)(rec & 1023u);
            const bool lg = (rec & kPrLong) != 0;
            if (lg ? idx < kl : idx < ks) return s_cnt[lg ? top - idx : idx];
            return idx < P.mcap ? tkz_result_cnt(ml[lg ? P.mcap - 1 - idx : idx]) : 1;
        };
        int running = 0, marks = 0;
#pragma unroll 1
        for (int kk = 0; kk < np && marks < dc; kk += 256) {
            // ---- 256 records: four consecutive ones a lane, one scan of tokens | marks << 20 ----
            const int k0 = kk + 4 * lane;
            uint32_t r[4] = {0u, 0u, 0u, 0u};
            if (k0 < np) {
                if (pb + k0 + 4 <= P.prank_cap) { const uint4 v = tkz_load16_nt(&P.prank[pb + k0]); r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w; }
                else for (int j = 0; j < 4; ++j) if (pb + k0 + j < P.prank_cap) r[j] = (uint32_t)P.prank[pb + k0 + j];
            }
            int c[4];
            bool mkd[4];
            int t = 0, mk = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = k0 + j < np && pb + k0 + j < P.prank_cap;
                const bool ms = ok && (r[j] & kPrMiss);
                if (all_kept) {                                  // (wave-uniform) without a branch: a hit reads the "one token" slot
                    const int idx = ((r[j] & kPrLong) ? top - (int)(r[j] & 1023u) : (int)(r[j] & 1023u)) & (kCountSlots - 1);
                    c[j] = ok ? s_cnt[ms ? idx : kCountSlots] : 0;
                } else c[j] = !ok ? 0 : ms ? miss_count(r[j]) : 1;
                if (promo && ok && !ms && (r[j] & kPromoFlag)) c[j] = (int)((r[j] >> kPromoCntShift) & 3u) + 1;
                mkd[j] = ok && (r[j] & kPrMark);
                t += c[j];
                mk += mkd[j] ? 1 : 0;
            }
            if (!simt::ballot(t > kCountLaneMax)) {
                int both;
                const int pre = tkz_wave_scan_sum(t | (mk << 20), &both);
                int pos = running + (pre & 0xFFFFF), mi = marks + (pre >> 20);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (mkd[j] && mi < dc) P.doc_tok[ord0 + mi] = pos;
                    mi += mkd[j] ? 1 : 0;
                    pos += c[j];
                }
                running += both & 0xFFFFF; marks += both >> 20;
                continue;
            }
            // ---- a chunk whose token sum may not fit 20 bits: 64 records at a time, as on k_place's general path ----
#pragma unroll 1
            for (int j = 0; j < 4 && marks < dc; ++j) {
                const int q0 = kk + 64 * j;
                if (q0 >= np) break;
                const int k = q0 + lane;
                const bool valid = k < np && pb + k < P.prank_cap;
                const uint32_t rec = valid ? (uint32_t)tkz_load_nt(&P.prank[pb + k]) : 0u;
                const bool miss = (rec & kPrMiss) != 0;
                int cnt = !valid ? 0 : miss ? miss_count(rec) : 1;
                if (promo && valid && !miss && (rec & kPromoFlag)) cnt = (int)((rec >> kPromoCntShift) & 3u) + 1;
                int tot;
                const int pos = running + tkz_wave_scan_sum(cnt, &tot);
                const bool marked = valid && (rec & kPrMark);
                const uint64_t mm = simt::ballot(marked);
                const int mi = marks + tkz_popc64(mm & tkz_lowmask(lane));
                if (marked && mi < dc) P.doc_tok[ord0 + mi] = pos;
                running += tot;
                marks += tkz_popc64(mm);
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------
// giant pieces (> kArenaPiece bytes: a run of thousands of letters, of '=' ...): found on the bitmap, merged by a whole
// 1024-thread workgroup each (tkz_bpe_long, rounds) before the encode kernels run
// -------------------------------------------------------------------------------------------------
// only a sub-tile k_probe flagged can hold the start of a giant piece, and only its LAST piece start can be one (a giant piece reaches past the
// end of its sub-tile): sub-tile t's, queued with its length (k_list_stats calls this for the flagged sub-tiles)
TKZ_DEV void tkz_giant_find_one(int64_t t, const uint64_t* startbits, int64_t nwords, int64_t total, int64_t* gq, unsigned long long* gcount, int64_t gcap) {
    int64_t p = -1;
    for (int k = kSub / 64 - 1; k >= 0 && p < 0; --k) {
        const int64_t w = t * (kSub / 64) + k;
        const uint64_t m = w < nwords ? startbits[w] : 0;
        if (m) p = (w << 6) + tkz_msb64(m);
    }
    if (p < 0 || p >= total) return;                         // (no piece starts here / the sentinel)
    int64_t next = total;
    for (int64_t v = (t + 1) * (kSub / 64); v < nwords; ++v) {
        const uint64_t x = startbits[v];
        if (x) { next = (v << 6) + tkz_ctz64(x); break; }
    }
    if (next - p > kArenaPiece) {
        const unsigned long long q = simt::atomic_add64(gcount, 1ull);
        if ((int64_t)q < gcap) { gq[2 * q] = p; gq[2 * q + 1] = next - p; }
    }
}
// The order the giant pieces are taken in: longest first (a diverse piece of tens of KiB is merged in thousands of rounds and sets the
// kernel's duration, so those must start first), by rank counting in one workgroup; identity beyond 8192 pieces.
constexpr int kGiantSort = 8192;
TKZ_KERNEL(1024) void k_giant_order(EncodeParams P) {
    if (tkz_attempt_failed(P)) return;
    TKZ_SHARED int32_t s_len[kGiantSort];
    const int64_t n = (int64_t)*P.giant_count < P.giant_cap ? (int64_t)*P.giant_count : P.giant_cap;
    int64_t* order = P.giant_q + 2 * P.giant_cap;
    if (n > kGiantSort) { for (int64_t i = simt::tid(); i < n; i += simt::nthreads()) order[i] = i; return; }
    for (int i = simt::tid(); i < (int)n; i += simt::nthreads()) { const int64_t l = P.giant_q[2 * i + 1]; s_len[i] = l > 0x7FFFFFFF ? 0x7FFFFFFF : (int32_t)l; }
    simt::sync();
    for (int i = simt::tid(); i < (int)n; i += simt::nthreads()) {
        const int32_t li = s_len[i];
        int rank = 0;
        for (int j = 0; j < (int)n; ++j) { const int32_t lj = s_len[j]; rank += (lj > li || (lj == li && j < i)) ? 1 : 0; }
        order[rank] = i;
    }
}

TKZ_KERNEL(1024) void k_giant_merge(TkzTables T, EncodeParams P) {
    if (tkz_attempt_failed(P)) return;
    TKZ_SHARED alignas(16) int32_t s_state[kBpeLongLdsBytes / 4];             // ids | pair ranks | flag bytes of up to 16 Ki parts + the tail's bounds: 152 KB of the CU's 160
    TKZ_SHARED int64_t s_off;
    TKZ_SHARED int32_t s_whole;
    TKZ_SHARED unsigned long long s_ticket;
    const int64_t n = (int64_t)*P.giant_count < P.giant_cap ? (int64_t)*P.giant_count : P.giant_cap;
    const int64_t* order = P.giant_q + 2 * P.giant_cap;
    int err = 0;
    // every workgroup keeps taking the next piece of the longest-first order until none is left (a fixed share per workgroup left the
    // ones with two long pieces working twice as long as the others)
    for (;;) {
        if (simt::tid() == 0) s_ticket = simt::atomic_add64(P.giant_ticket, 1ull);
        simt::sync();
        const int64_t t = (int64_t)s_ticket;
        simt::sync();
        if (t >= n) break;
        const int64_t q = order[t];
        const int64_t p = P.giant_q[2 * q], len64 = P.giant_q[2 * q + 1];
        int cnt = 0;
        if (len64 > kMaxPiece) err |= kErrTooLong;
        else {
            const int len = (int)len64;
            const uint8_t* gb = P.bytes + p;
            auto at = [&](int i) -> uint32_t { return gb[i]; };
            int32_t* dst = P.tmp + p;
            if (simt::tid() == 0) {
                s_whole = tkz_lookup_long(T, at, (uint32_t)len);                 // TikTokenizer.cs:262 (a key this long is unusual, not impossible)
                const unsigned long long need = 6ull * (unsigned long long)len;
                const unsigned long long o = simt::atomic_add64(P.pool_head, need);
                s_off = (o + need <= (unsigned long long)P.pool_cap) ? (int64_t)o : -1;
            }
            simt::sync();
            const int32_t whole = s_whole;
            const int64_t off = s_off;
            simt::sync();
            if (whole != TKZ_RANK_NONE) { if (simt::tid() == 0) dst[0] = whole; cnt = 1; }
            else if (off < 0) { err |= kErrPool; cnt = -1; }
            else {
                int32_t* arr = P.pool + off;
                cnt = tkz_bpe_long(T, at, len, arr, arr + len, arr + 2 * (int64_t)len, arr + 3 * (int64_t)len, arr + 4 * (int64_t)len, arr + 5 * (int64_t)len, dst, &err, s_state, TKZ_DEV_FLAG(P, 16) ? P.devprof : nullptr);
            }
        }
        if (simt::tid() == 0) P.giant_cnt[p / kSub] = cnt;
        simt::sync();
    }
    if (err) simt::atomic_or((unsigned*)&P.counters[0], (unsigned)err);
}

// documents and pieces that start in each sub-tile (for their ordinals), the two bitmaps in one pass (the words of both read by the same lane)
TKZ_KERNEL(256) void k_doccount2(const uint64_t* bits_a, const uint64_t* bits_b, int64_t nwords, int64_t total, int64_t nsub, int32_t* cnt_a, int32_t* cnt_b) {
    static_assert(kSub / 64 == 16, "k_doccount2 sums 16 lanes per sub-tile");
    const int lane = simt::lane();
    const int64_t stride = simt::nblocks() * simt::nthreads(), nw = nsub * (kSub / 64);
    for (int64_t w0 = simt::bid() * simt::nthreads() + (simt::tid() & ~63); w0 < nw; w0 += stride) {
        const int64_t w = w0 + lane;
        uint64_t ma = (w < nw && w < nwords) ? bits_a[w] : 0ull, mb = (w < nw && w < nwords) ? bits_b[w] : 0ull;
        const int64_t lim = total - (w << 6);              // (the sentinel bit at `total` is not a start)
        if (lim <= 0) { ma = 0; mb = 0; } else if (lim < 64) { ma &= tkz_lowmask((int)lim); mb &= tkz_lowmask((int)lim); }
        int c = tkz_popc64(ma) | (tkz_popc64(mb) << 16);  // (at most 1024 of either in a sub-tile: the two sums share the shuffles)
        c += simt::shfl_xor(c, 1); c += simt::shfl_xor(c, 2); c += simt::shfl_xor(c, 4); c += simt::shfl_xor(c, 8);
        if ((lane & 15) == 0 && w < nw) { cnt_a[w >> 4] = c & 0xFFFF; cnt_b[w >> 4] = c >> 16; }
    }
}

// -------------------------------------------------------------------------------------------------
// exclusive scan of tile_count (int32) -> tile_base (int64); counters[2..3] (int64) = grand total
// -------------------------------------------------------------------------------------------------
// Up to kScanSmallMax sub-tiles: ONE workgroup, one launch -- a thread owns n / 1024 consecutive counts, one workgroup scan of the
// threads' sums -- for one or two arrays at once; the three-kernel form below (partials, top, final) costs three dependent launches per array, and a
// batch of a few megabytes is made of little else than launches.
constexpr int kScanSmallMax = 8192;          // (8 MB of text.  At 65,536 sub-tiles the one workgroup took 35 us a scan against 17 us for the three kernels: measured on the 64 MB single document of --kind 5)
TKZ_KERNEL(1024) void k_scan_small(const int32_t* cnt_a, int64_t* base_a, int64_t* grand_a, int round_a,
                                   const int32_t* cnt_b, int64_t* base_b, int64_t* grand_b, int round_b, int n) {
    const int tid = simt::tid(), nth = simt::nthreads();
    const int per = (n + nth - 1) / nth, lo = tid * per, hi = lo + per < n ? lo + per : n;
    for (int arr = 0; arr < 2; ++arr) {
        const int32_t* cnt = arr ? cnt_b : cnt_a;
        int64_t* base = arr ? base_b : base_a;
        int64_t* grand = arr ? grand_b : grand_a;
        const int round = arr ? round_b : round_a;
        if (!cnt) continue;                                   // (workgroup-uniform)
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += (cnt[i] + round) & ~round;
        int tot;
        int run = tkz_block_scan(sum, &tot);                  // (<= 1024 per sub-tile, <= 65536 sub-tiles: 2^26 at most)
        for (int i = lo; i < hi; ++i) { base[i] = run; run += (cnt[i] + round) & ~round; }
        if (tid == 0 && grand) *grand = tot;
        simt::sync();
    }
}
// (`round`: every count is rounded up to a multiple of round + 1 first -- the piece records of a sub-tile are whole 64-byte lines)
TKZ_KERNEL(256) void k_scan_partials(const int32_t* cnt, int64_t n, int64_t* bsum, int round) {
    TKZ_SHARED int64_t s_w[4];
    const int64_t i0 = simt::bid() * kScanBlock;
    int64_t v = 0;
    for (int j = simt::tid(); j < kScanBlock; j += kThreads) if (i0 + j < n) v += (cnt[i0 + j] + round) & ~round;
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = simt::shflu((uint32_t)v, simt::lane() ^ d), hi = simt::shflu((uint32_t)((uint64_t)v >> 32), simt::lane() ^ d);
        v += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    if (simt::lane() == 0) s_w[simt::wave()] = v;
    simt::sync();
    if (simt::tid() == 0) bsum[simt::bid()] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
TKZ_KERNEL(256) void k_scan_top(int64_t* bsum, int64_t nblk, int64_t* grand) {   // one workgroup, kThreads partial sums per step
    TKZ_SHARED int64_t s_w[kThreads / 64];
    const int lane = simt::lane(), wave = simt::wave();
    int64_t carry = 0;
    for (int64_t i0 = 0; i0 < nblk; i0 += kThreads) {
        const int64_t i = i0 + simt::tid();
        const int64_t v = i < nblk ? bsum[i] : 0;
        int64_t x = v;                                   // inclusive scan inside the wavefront
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t lo = simt::shflu((uint32_t)x, lane - d < 0 ? lane : lane - d);
            const uint32_t hi = simt::shflu((uint32_t)((uint64_t)x >> 32), lane - d < 0 ? lane : lane - d);
            if (lane >= d) x += (int64_t)(((uint64_t)hi << 32) | lo);
        }
        if (lane == 63) s_w[wave] = x;
        simt::sync();
        int64_t woff = 0, tot = 0;
        for (int w = 0; w < kThreads / 64; ++w) { const int64_t t = s_w[w]; if (w < wave) woff += t; tot += t; }
        simt::sync();
        if (i < nblk) bsum[i] = carry + woff + x - v;
        carry += tot;
    }
    if (simt::tid() == 0) *grand = carry;
}
TKZ_KERNEL(256) void k_scan_final(const int32_t* cnt, int64_t n, const int64_t* boff, int64_t* base, int round) {
    const int64_t i0 = simt::bid() * kScanBlock;
    // each thread owns kScanBlock/kThreads consecutive tiles
    constexpr int per = kScanBlock / kThreads;
    int local[per]; int sum = 0;
    for (int j = 0; j < per; ++j) { const int64_t i = i0 + (int64_t)simt::tid() * per + j; local[j] = i < n ? (cnt[i] + round) & ~round : 0; sum += local[j]; }
    // block scan in 64-bit via two 32-bit scans would overflow only past 2^31 tokens per 1024 tiles (4 MiB of text): impossible
    int tot;
    int pre = tkz_block_scan(sum, &tot);
    int64_t run = boff[simt::bid()] + pre;
    for (int j = 0; j < per; ++j) { const int64_t i = i0 + (int64_t)simt::tid() * per + j; if (i < n) base[i] = run; run += local[j]; }
}

// -------------------------------------------------------------------------------------------------
// k_docoffs
// -------------------------------------------------------------------------------------------------
// (c3a / c3b / c3c: null, or blocks that receive {c3_docs, total, *grand} -- the batch's counts, k_counts3's job, by the first thread: one launch less)
// The ordinal of item d's mark.  The marks are the DISTINCT start positions below `total`, and k_place / k_tokcount fill doc_tok by a mark's ordinal among
// them.  When no item of the batch is empty (*has_empty == 0: k_docmark saw offs[d] < offs[d + 1] for every d < n_docs) the offsets increase strictly on
// [0, n_docs], so the starts below `total` are exactly items 0 .. n_docs - 1, all distinct and in order: the mark of item d has ordinal d, and neither the
// bitmap nor docord_base is read.  (Offsets that are not monotone fail the batch in k_docmark; d <= n_docs < the n_docs + 2 entries of doc_tok whatever they
// say.)  At piece granularity the items are the piece starts as k_piece_index read them off the bitmap: distinct by construction, so the same holds; a batch
// with an empty document takes the search there too.  With an empty item several items share a mark, and the ordinal is searched as before.
TKZ_KERNEL(256) void k_docoffs(const int64_t* offs, int64_t n_docs, int64_t total, const int64_t* tile_base, const uint64_t* docbits,
                               const int64_t* docord_base, const int32_t* doc_tok, const int64_t* grand, int64_t* out_offs,
                               int64_t c3_docs, int64_t* c3a, int64_t* c3b, int64_t* c3c, const int32_t* has_empty) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    const bool search = *has_empty != 0;                // (one word for the whole grid: wave-uniform)
    if (simt::bid() == 0 && simt::tid() == 0) {
        const int64_t g = *grand;
        if (c3a) { c3a[0] = c3_docs; c3a[1] = total; c3a[2] = g; }
        if (c3b) { c3b[0] = c3_docs; c3b[1] = total; c3b[2] = g; }
        if (c3c) { c3c[0] = c3_docs; c3c[1] = total; c3c[2] = g; }
    }
    for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d <= n_docs; d += stride) {
        const int64_t pos = offs[d];
        if (pos >= total) { out_offs[d] = *grand; continue; }
        if (pos < 0) { out_offs[d] = 0; continue; }
        const int64_t sub = pos / kSub, wpos = pos >> 6;
        if (!search) { out_offs[d] = tile_base[sub] + doc_tok[d]; continue; }
        int64_t ord = docord_base[sub];
        for (int64_t w = sub * (kSub / 64); w < wpos; ++w) ord += tkz_popc64(docbits[w]);
        ord += tkz_popc64(docbits[wpos] & tkz_lowmask((int)(pos & 63)));
        out_offs[d] = tile_base[sub] + doc_tok[ord];
    }
}

// TKZ_OPT_CASE_EQUIVALENCE (cl100k on a .NET >= 7 host): `(?i:'s|'t|...)` there is matched with the runtime's case-equivalence tables, under which
// U+017F (LATIN SMALL LETTER LONG S, bytes C5 BF) is an `s`: an apostrophe at which a match starts, followed by U+017F, IS the contraction -- the piece
// ends behind the long s.  Every scanner treats U+017F as the letter it is (net6.0: ASCII case pairs only; the apostrophe is then the one-char prefix
// of the word that follows), so the only difference is one more piece start: right behind the long s.  This pass over the text adds it, whichever scanner
// wrote the bitmap.  (None of the other letters of the seven literals has a non-ASCII equivalent: U+212A KELVIN SIGN is a `k`.)
TKZ_KERNEL(256) void k_case_equiv_fix(const uint8_t* bytes, int64_t total, const uint64_t* docbits, uint64_t* startbits) {
    const int64_t stride = simt::nblocks() * simt::nthreads() * 8;
    for (int64_t i0 = (simt::bid() * (int64_t)simt::nthreads() + simt::tid()) * 8; i0 < total; i0 += stride) {
        uint64_t w = 0;                                      // (bytes is 16-byte aligned; nothing is read beyond `total`)
        if (i0 + 8 <= total) w = *reinterpret_cast<const uint64_t*>(bytes + i0);
        else for (int k = 0; i0 + k < total; ++k) w |= (uint64_t)bytes[i0 + k] << (8 * k);
        const uint64_t x = w ^ 0x2727272727272727ull;
        if (!((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull)) continue;      // no apostrophe among these eight bytes
        for (int k = 0; k < 8; ++k) {
            const int64_t i = i0 + k;
            if (i + 3 > total || ((w >> (8 * k)) & 0xFFu) != 0x27u) continue;
            if (bytes[i + 1] != 0xC5u || bytes[i + 2] != 0xBFu) continue;
            if (!((startbits[i >> 6] >> (i & 63)) & 1ull)) continue;                     // no match starts at the apostrophe
            if (((docbits[(i + 1) >> 6] >> ((i + 1) & 63)) & 1ull) || ((docbits[(i + 2) >> 6] >> ((i + 2) & 63)) & 1ull)) continue;   // (the document ends behind the apostrophe)
            simt::atomic_or64((unsigned long long*)&startbits[(i + 3) >> 6], 1ull << ((i + 3) & 63));
        }
    }
}

// -------------------------------------------------------------------------------------------------
// Special tokens (the special entries): EncodeInternal / FindNextSpecialToken (TikTokenizer.cs:141-170,230-241) for a batch.
//   k_lit_scan     position-parallel over the text: at byte p "the match" is the FIRST registered literal whose bytes are the text at p and that ends inside
//                  p's document (the reference's alternation); p is a CANDIDATE when that literal is allowed.  One wavefront per 4 KiB, staged in LDS with
//                  the literal table; a lane looks at a byte, the 256-bit set of first bytes sends nearly all of them on.
//   k_lit_resolve  the literals TAKEN: left to right inside a document, the first candidate at or after the end of the one before.  A candidate no other
//                  candidate reaches over is taken whatever came before it: it heads a RUN, which one lane walks to the next head (one step for literals
//                  that do not overlap -- every `<|endoftext|>` of a corpus heads its own run).  Starts and ends are OR-ed into the bitmaps.
//   k_lit_fix      behind the pre-tokenizer (which split every stretch between segment marks -- the taken literals too -- as a text of its own): the piece
//                  starts strictly inside a taken literal are cleared, so that it is ONE piece; k_probe_special makes that piece's record the literal's id.
// -------------------------------------------------------------------------------------------------
// bytes from p to the end of p's document (the next document mark behind p; the bitmap ends in a mark at `total`), or kLitMaxLen + 1 when that is further away
// (never more than the text holds, whatever the bitmap says: offsets that k_docmark refused leave it without its last mark)
TKZ_DEV int tkz_lit_room(const uint64_t* docbits, int64_t nwords, int64_t total, int64_t p) {
    const int64_t w = p >> 6;
    const int b = (int)(p & 63);
    int r = kLitMaxLen + 1;
    uint64_t m = b == 63 ? 0ull : docbits[w] >> (b + 1);
    if (m) r = tkz_ctz64(m) + 1;
    else if ((m = w + 1 < nwords ? docbits[w + 1] : 0ull) != 0) r = 64 - b + tkz_ctz64(m);
    else if ((m = w + 2 < nwords ? docbits[w + 2] : 0ull) != 0) r = 128 - b + tkz_ctz64(m);
    return total - p < r ? (int)(total - p) : r;
}
// the first registered literal of at most `room` bytes whose bytes are tx[0 ..): its index, or -1.  rw: null, or replaced-byte bitmap words (nrw of them) in
// which tx[0] is bit `rbit`: a literal that holds U+FFFD does not match over a byte the transcoder put there for a lone surrogate.  (The words are read from
// memory, by k_lit_scan too, and only once ALL bytes of such a literal have matched: staging 66 words a wavefront beside k_lit_scan's text would take its
// workgroup from 51.8 KB to 53.9 KB of LDS -- past a third of the CU's 160 KB once rounded to the allocation granule, two workgroups a CU instead of three,
// for every special call, UTF-8 ones included.)
TKZ_DEV int tkz_lit_first(const uint32_t* meta, const uint8_t* blob, int n, const uint8_t* tx, int room, const uint64_t* rw, int64_t nrw, int64_t rbit) {
    for (int i = 0; i < n; ++i) {
        const uint32_t m = meta[kLitMetaHead + 2 * i];
        const int len = (int)(m >> 16);
        if (len > room) continue;
        const uint8_t* lit = blob + (m & 0xFFFFu);
        int k = 0;
        while (k < len && lit[k] == tx[k]) ++k;
        if (k == len && !tkz_lit_replaced(meta, i, rw, nrw, rbit, len)) return i;
    }
    return -1;
}
constexpr int kLitBlock = 4096;                            // bytes of text per wavefront of k_lit_scan (64 bitmap words)
constexpr int kLitTextQuads = (kLitBlock + kLitMaxLen) / 16;
constexpr int kLitMetaWords = kLitMetaHead + 2 * kLitMax, kLitBlobQuads = kLitMax * kLitMaxLen / 16;
// the literal table (a few hundred bytes as a rule) into LDS, by the whole workgroup; the caller's barrier follows
TKZ_DEV void tkz_lit_stage_table(const TkzLitTable& LT, uint32_t* s_meta, uint4* s_blob) {
    uint8_t* sb = reinterpret_cast<uint8_t*>(s_blob);
    for (int i = simt::tid(); i < kLitMetaHead + 2 * LT.n; i += simt::nthreads()) s_meta[i] = LT.meta[i];
    for (int i = simt::tid(); i < LT.blob_bytes; i += simt::nthreads()) sb[i] = LT.blob[i];
}
// block `blk` of BLOCK bytes of text by ONE wavefront (k_lit_scan: a wavefront of each workgroup; k_small: the blocks dealt out to its wavefronts): its candidate
// words, and the words of the three bitmaps k_lit_resolve ORs into as they start out.  tq: (BLOCK + kLitMaxLen) / 16 quads of LDS of the wavefront's own.
template <int BLOCK>
TKZ_DEV void tkz_lit_scan_block(int64_t blk, uint4* tq, const uint32_t* s_meta, const uint4* s_blob, const uint8_t* bytes, int64_t total, const uint64_t* docbits,
                                int64_t nwords, int n_lit, const TkzLitAllowed& A, uint64_t* candbits, uint64_t* segbits, uint64_t* specbits, uint64_t* endbits,
                                const uint64_t* repl) {
    static_assert(BLOCK % 64 == 0 && BLOCK / 64 <= 64 && (BLOCK + kLitMaxLen) % 16 == 0, "a lane keeps a bitmap word of the block");
    const int lane = simt::lane();
    const int64_t w0 = blk * (BLOCK / 64), base = blk * BLOCK;
    if (w0 >= nwords) return;
    for (int q = lane; q < (BLOCK + kLitMaxLen) / 16; q += 64) {       // the block and the bytes a literal that starts in it may reach; zeros beyond the text
        const int64_t p = base + 16 * (int64_t)q;
        uint4 v; v.x = v.y = v.z = v.w = 0;
        if (p + 16 <= total) v = tkz_load16_nt(bytes + p);
        else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (int k = 0; k < 16; ++k) if (p + k < total) w[k >> 2] |= (uint32_t)bytes[p + k] << (8 * (k & 3));
            v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        }
        tq[q] = v;
    }
    (void)simt::ballot(true);
    const uint8_t* const tx = reinterpret_cast<const uint8_t*>(tq);
    const uint8_t* const blob = reinterpret_cast<const uint8_t*>(s_blob);
    uint64_t mine = 0;                                     // lane j keeps word w0 + j
#pragma unroll 1
    for (int j = 0; j < BLOCK / 64; ++j) {
        if (w0 + j >= nwords) break;                       // (wave-uniform)
        const int pos = 64 * j + lane;
        const int64_t p = base + pos;
        const uint32_t c = tx[pos];
        bool cand = false;
        if (p < total && ((s_meta[c >> 5] >> (c & 31)) & 1u)) {
            const int i = tkz_lit_first(s_meta, blob, n_lit, tx + pos, tkz_lit_room(docbits, nwords, total, p), repl, nwords, p);
            cand = i >= 0 && ((A.m[i >> 6] >> (i & 63)) & 1ull);
        }
        const uint64_t m = simt::ballot(cand);
        if (lane == j) mine = m;
    }
    const int64_t w = w0 + lane;
    if (lane < BLOCK / 64 && w < nwords) { candbits[w] = mine; segbits[w] = docbits[w]; specbits[w] = 0; endbits[w] = 0; }
}
TKZ_KERNEL(256) void k_lit_scan(const uint8_t* bytes, int64_t total, const uint64_t* docbits, int64_t nwords, TkzLitTable LT, TkzLitAllowed A,
                                uint64_t* candbits, uint64_t* segbits, uint64_t* specbits, uint64_t* endbits, const uint64_t* repl) {
    TKZ_SHARED uint4 s_text[kThreads / 64][kLitTextQuads];
    TKZ_SHARED uint32_t s_meta[kLitMetaWords];
    TKZ_SHARED uint4 s_blob[kLitBlobQuads];
    tkz_lit_stage_table(LT, s_meta, s_blob);
    simt::sync();
    tkz_lit_scan_block<kLitBlock>(simt::bid() * (kThreads / 64) + simt::wave(), s_text[simt::wave()], s_meta, s_blob, bytes, total, docbits, nwords, LT.n, A,
                                  candbits, segbits, specbits, endbits, repl);
}
// the literal that k_lit_scan matched at candidate p (from the text: candidates are rare): its length
TKZ_DEV int tkz_lit_len_at(const uint8_t* bytes, const uint64_t* docbits, int64_t nwords, int64_t total, const TkzLitTable& LT, int64_t p, const uint64_t* repl) {
    const int i = tkz_lit_first(LT.meta, LT.blob, LT.n, bytes + p, tkz_lit_room(docbits, nwords, total, p), repl, nwords, p);
    return i < 0 ? 1 : (int)(LT.meta[kLitMetaHead + 2 * i] >> 16);
}
// does a candidate in front of p reach over p?  (Only one that starts within kLitMaxLen - 1 bytes can; the nearest first: in a run of overlapping literals it does.)
TKZ_DEV bool tkz_lit_covered(const uint8_t* bytes, const uint64_t* docbits, const uint64_t* candbits, int64_t nwords, int64_t total, const TkzLitTable& LT, int64_t p, const uint64_t* repl) {
    const int64_t lo = p - (kLitMaxLen - 1) > 0 ? p - (kLitMaxLen - 1) : 0;
    for (int64_t w = (p - 1) >> 6; p > 0 && w >= (lo >> 6); --w) {
        uint64_t m = candbits[w];
        if (w == ((p - 1) >> 6)) m &= tkz_lowmask((int)((p - 1) & 63) + 1);
        if (w == (lo >> 6)) m &= ~tkz_lowmask((int)(lo & 63));
        while (m) {
            const int b = tkz_msb64(m);
            m &= ~(1ull << b);
            const int64_t q = (w << 6) + b;
            if (q + tkz_lit_len_at(bytes, docbits, nwords, total, LT, q, repl) > p) return true;
        }
    }
    return false;
}
// bitmap word w by ONE thread: the runs its candidates head, walked; the number of literals taken
TKZ_DEV unsigned long long tkz_lit_resolve_word(int64_t w, const uint8_t* bytes, int64_t total, const uint64_t* docbits, const uint64_t* candbits, int64_t nwords,
                                                const TkzLitTable& LT, uint64_t* segbits, uint64_t* specbits, uint64_t* endbits, const uint64_t* repl) {
    unsigned long long taken = 0;
    for (uint64_t m = candbits[w]; m; m &= m - 1) {
        const int64_t head = (w << 6) + tkz_ctz64(m);
        if (tkz_lit_covered(bytes, docbits, candbits, nwords, total, LT, head, repl)) continue;       // (another lane's run)
        for (int64_t cur = head; cur >= 0;) {
            const int64_t end = cur + tkz_lit_len_at(bytes, docbits, nwords, total, LT, cur, repl);    // (<= total: the literal ends inside its document)
            simt::atomic_or64((unsigned long long*)&specbits[cur >> 6], 1ull << (cur & 63));
            simt::atomic_or64((unsigned long long*)&endbits[end >> 6], 1ull << (end & 63));
            simt::atomic_or64((unsigned long long*)&segbits[cur >> 6], 1ull << (cur & 63));
            simt::atomic_or64((unsigned long long*)&segbits[end >> 6], 1ull << (end & 63));
            ++taken;
            // the next candidate at or after `end`: part of this run when a candidate in front of it reaches over it -- it then starts less than kLitMaxLen
            // bytes behind `end` --, the head of a run of its own otherwise
            int64_t nxt = -1;
            for (int64_t v = end >> 6; v < nwords && v <= (end + kLitMaxLen) >> 6 && nxt < 0; ++v) {
                uint64_t c = candbits[v];
                if (v == (end >> 6)) c &= ~tkz_lowmask((int)(end & 63));
                if (c) nxt = (v << 6) + tkz_ctz64(c);
            }
            cur = nxt >= 0 && nxt < total && tkz_lit_covered(bytes, docbits, candbits, nwords, total, LT, nxt, repl) ? nxt : -1;
        }
    }
    return taken;
}
TKZ_KERNEL(256) void k_lit_resolve(const uint8_t* bytes, int64_t total, const uint64_t* docbits, const uint64_t* candbits, int64_t nwords, TkzLitTable LT,
                                   uint64_t* segbits, uint64_t* specbits, uint64_t* endbits, unsigned long long* n_taken, const uint64_t* repl) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    unsigned long long taken = 0;
    for (int64_t w = simt::bid() * simt::nthreads() + simt::tid(); w < nwords; w += stride)
        taken += tkz_lit_resolve_word(w, bytes, total, docbits, candbits, nwords, LT, segbits, specbits, endbits, repl);
    if (taken) simt::atomic_add64(n_taken, taken);
}
// one bitmap word a lane.  `inside` = the bytes strictly inside a taken literal: the running XOR of a mark behind every start and one at every end (a literal of
// one byte: the two cancel); what is open at the word's first bit comes from the last start in the 128 bytes before it.
TKZ_DEV void tkz_lit_fix_word(int64_t w, uint64_t* startbits, const uint64_t* segbits, const uint64_t* specbits, const uint64_t* endbits) {
    static_assert(kLitMaxLen <= 128, "a literal spans at most three bitmap words");
    const uint64_t s0 = specbits[w], e0 = endbits[w];
    const uint64_t s1 = w > 0 ? specbits[w - 1] : 0ull, e1 = w > 0 ? endbits[w - 1] : 0ull;
    bool open = false;                                 // byte 64 w - 1 is inside a literal that goes on into this word
    const uint64_t s1lo = s1 & ~(1ull << 63);
    if (s1lo) { const int b = tkz_msb64(s1lo); open = (e1 >> (b + 1)) == 0; }
    else if (w > 1 && specbits[w - 2]) {
        const int b = tkz_msb64(specbits[w - 2]);
        open = ((b == 63 ? 0ull : endbits[w - 2] >> (b + 1)) | e1) == 0;
    }
    uint64_t x = ((s0 << 1) | (s1 >> 63)) ^ e0;
    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
    if (open) x = ~x;
    if (x | segbits[w]) startbits[w] = (startbits[w] & ~x) | segbits[w];
}
TKZ_KERNEL(256) void k_lit_fix(uint64_t* startbits, const uint64_t* segbits, const uint64_t* specbits, const uint64_t* endbits, int64_t nwords) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    for (int64_t w = simt::bid() * simt::nthreads() + simt::tid(); w < nwords; w += stride) tkz_lit_fix_word(w, startbits, segbits, specbits, endbits);
}

// document offsets of a chunk cut out of a larger batch: made relative to the chunk's first byte
// A small host batch on page-locked buffers: the text and the offsets come over PCIe by this kernel's own loads (they are device-visible), into the
// staging buffers the other kernels read, and the workspace's zero region is cleared by the same launch -- in place of two copy commands, two fills and
// the stream hand-over between them (68 us before the first kernel of a 1 MB call; this is ~25).  h_bytes 16-byte aligned.
TKZ_KERNEL(256) void k_ingest(const uint8_t* h_bytes, int64_t total, uint8_t* d_bytes, const int64_t* h_offs, int64_t n_offs, int64_t* d_offs, uint4* zero, int64_t zero_quads) {
    const int64_t i0 = (int64_t)simt::bid() * simt::nthreads() + simt::tid(), stride = (int64_t)simt::nblocks() * simt::nthreads();
    const int64_t full = total >> 4;
    for (int64_t i = i0; i < full; i += stride) *reinterpret_cast<uint4*>(d_bytes + 16 * i) = tkz_load16(h_bytes + 16 * i);
    for (int64_t i = (full << 4) + i0; i < total; i += stride) d_bytes[i] = h_bytes[i];          // (nothing is read beyond the caller's buffer)
    for (int64_t i = i0; i < n_offs; i += stride) d_offs[i] = h_offs[i];
    const uint4 z = {0u, 0u, 0u, 0u};
    for (int64_t i = i0; i < zero_quads; i += stride) zero[i] = z;
}
TKZ_KERNEL(256) void k_rebase(int64_t* offs, int64_t n, int64_t base) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    for (int64_t i = simt::bid() * simt::nthreads() + simt::tid(); i < n; i += stride) offs[i] -= base;
}

// What the miss lists of the batch needed, from a pass over mcount (a few atomics per workgroup; k_probe used to keep these itself, every wavefront
// reading -- and many updating -- ONE line of the counter block: 8 ms of a miss-heavy batch, 100 ms of a batch whose lists all overflow):
//   counters[0] |= kErrMissCap, counters[1] = the longest list, when some list did not fit mcap (the host grows the lists and runs the batch again);
//   counters[2] = the longest list above kMissCapMin that did fit (the host lets grown lists shrink again by it);
//   counters[3] = how many sub-tiles hold more than 64 entries (the host picks k_place's form for the workspace's next batch by it).
// (... and, in the same pass over the sub-tiles, k_giant_find's: a sub-tile k_probe flagged as holding a giant piece queues it -- one launch less)
TKZ_KERNEL(256) void k_list_stats(const uint32_t* mcount, int64_t nsub, int32_t mcap, int32_t* counters,
                                  const uint8_t* heavy_flag, const uint64_t* startbits, int64_t nwords, int64_t total, int64_t* gq, unsigned long long* gcount, int64_t gcap,
                                  const uint32_t* mlist, uint64_t* coop_q, unsigned long long* coop_count, int64_t coop_cap, int lane_piece, unsigned long long* miss_sums) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    const int lane = simt::lane();
    int mx = 0, big = 0, over = 0;
    long long n_short = 0, n_long = 0;       // (miss_sums: what the batch's pieces missed -- the host follows that share from batch to batch, TKZ_OPT_ADAPT)
    for (int64_t i0 = simt::bid() * simt::nthreads() + (simt::tid() & ~63); i0 < nsub; i0 += stride) {      // (wave-uniform: the queueing below is a wave scan)
        const int64_t i = i0 + lane;
        const bool in = i < nsub;
        const uint32_t m = in ? mcount[i] : 0u;
        const int n = (int)(m & 0xFFFFu) + (int)(m >> 16);
        n_short += (int)(m & 0xFFFFu); n_long += (int)(m >> 16);
        if (n <= mcap) { if (n > mx) mx = n; } else if (n > big) big = n;
        over += n > 64 ? 1 : 0;
        const uint32_t hf = in ? heavy_flag[i] : 0u;
        if (hf & 2u) tkz_giant_find_one(i, startbits, nwords, total, gq, gcount, gcap);
        // the long misses of more than kLanePiece bytes (k_probe flagged their sub-tiles: bit 2) are queued for k_merge_coop: sub-tile << 10 | index in
        // its long list.  One atomic per wavefront of 64 sub-tiles, not per piece.
        if (simt::ballot((hf & 4u) != 0)) {
            const int nl = (int)(m >> 16);
            int mine = 0;
            // (four entries a step, their loads requested together: a lane walks its sub-tile's long list alone -- real text has lists of forty entries, one
            //  round trip each was 139 us of this kernel on 268 MB)
            const uint32_t* const top = mlist + i * (int64_t)mcap + (mcap - 1);
            const bool walk = (hf & 4u) && n <= mcap;
            if (walk)
                for (int j = 0; j < nl; j += 4) {
                    uint32_t ent[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) ent[k] = j + k < nl ? top[-(j + k)] : 0u;
#pragma unroll
                    for (int k = 0; k < 4; ++k) mine += ((int)((ent[k] >> kMrLenShift) & 1023u) + 1 > lane_piece) ? 1 : 0;
                }
            int tot;
            const int pre = tkz_wave_scan_sum(mine, &tot);
            unsigned long long base = 0;
            if (lane == 0 && tot) base = simt::atomic_add64(coop_count, (unsigned long long)tot);
            base = ((unsigned long long)simt::shflu((uint32_t)(base >> 32), 0) << 32) | simt::shflu((uint32_t)base, 0);
            if (mine) {
                unsigned long long at = base + (unsigned long long)pre;
                for (int j = 0; j < nl; j += 4) {
                    uint32_t ent[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) ent[k] = j + k < nl ? top[-(j + k)] : 0u;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if ((int)((ent[k] >> kMrLenShift) & 1023u) + 1 > lane_piece) { if ((int64_t)at < coop_cap) coop_q[at] = ((uint64_t)i << 10) | (uint64_t)(j + k); ++at; }
                }
            }
        }
    }
    int tot;
    (void)tkz_wave_scan_sum(over, &tot);
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = simt::shfl(mx, simt::lane() ^ d), b = simt::shfl(big, simt::lane() ^ d);
        mx = o > mx ? o : mx; big = b > big ? b : big;
    }
    // (64-bit sums over the wave by two 32-bit scans: a wavefront's share is far below 2^31)
    int ts = 0, tl = 0;
    if (miss_sums) { (void)tkz_wave_scan_sum((int)n_short, &ts); (void)tkz_wave_scan_sum((int)n_long, &tl); }
    // One set of atomics a WORKGROUP: its four wavefronts meet in LDS first.  (A set per wavefront was 4,096 x 6 atomics on the same few words: ~110 us of this
    // kernel whatever the batch -- 268 MB of real text or the 5 GB headline.)
    TKZ_SHARED int s_red[kThreads / 64][5];
    if (simt::lane() == 0) { int* r = s_red[simt::wave()]; r[0] = big; r[1] = mx; r[2] = tot; r[3] = ts; r[4] = tl; }
    simt::sync();
    if (simt::tid() == 0) {
        long long sum_s = 0, sum_l = 0;
        big = 0; mx = 0; tot = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            const int* r = s_red[w];
            big = r[0] > big ? r[0] : big; mx = r[1] > mx ? r[1] : mx; tot += r[2]; sum_s += r[3]; sum_l += r[4];
        }
        if (big) { simt::atomic_or((unsigned*)&counters[0], (unsigned)kErrMissCap); simt::atomic_max((unsigned*)&counters[1], (unsigned)big); }
        if (mx > kMissCapMin) simt::atomic_max((unsigned*)&counters[2], (unsigned)mx);
        if (tot) simt::atomic_add(&counters[3], tot);
        if (miss_sums && (sum_s | sum_l)) { simt::atomic_add64(&miss_sums[0], (unsigned long long)sum_s); simt::atomic_add64(&miss_sums[1], (unsigned long long)sum_l); }
    }
}

// TKZ_OPT_PIECE_STATS: the lengths of the miss lists of all sub-tiles, summed (short | long << 16 per sub-tile)
TKZ_KERNEL(256) void k_miss_stats(const uint32_t* mcount, const int32_t* pcount, int64_t nsub, unsigned long long* stats) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    int ns = 0, nl = 0, np = 0;
    for (int64_t i = simt::bid() * simt::nthreads() + simt::tid(); i < nsub; i += stride) { const uint32_t m = mcount[i]; ns += (int)(m & 0xFFFFu); nl += (int)(m >> 16); np += pcount[i]; }
    int ts, tl, tp;
    (void)tkz_wave_scan_sum(ns, &ts);
    (void)tkz_wave_scan_sum(nl, &tl);
    (void)tkz_wave_scan_sum(np, &tp);
    if (simt::lane() == 0 && (ts | tl | tp)) {
        simt::atomic_add64(&stats[2], (unsigned long long)ts); simt::atomic_add64(&stats[3], (unsigned long long)tl); simt::atomic_add64(&stats[4], (unsigned long long)tp);
    }
}

// {n_docs, n_bytes, n_tokens} of the batch, on the device: what tkz_comm_allgather_counts_device sends (no host round trip)
// (up to three copies: the encoder's "last batch" block, the workspace's block of THIS batch, a block of the caller's)
TKZ_KERNEL(64) void k_counts3(int64_t n_docs, int64_t total, const int64_t* grand, int64_t* out3, int64_t* out3b, int64_t* out3c) {
    if (simt::tid() == 0) {
        const int64_t g = grand ? *grand : 0;
        out3[0] = n_docs; out3[1] = total; out3[2] = g;
        if (out3b) { out3b[0] = n_docs; out3b[1] = total; out3b[2] = g; }
        if (out3c) { out3c[0] = n_docs; out3c[1] = total; out3c[2] = g; }
    }
}

// -------------------------------------------------------------------------------------------------
// UTF-16 documents -> UTF-8 documents on the device (the batch form of Encoding.UTF8.GetBytes, TikTokenizer.cs:261):
// a host whose strings are UTF-16 (.NET, Java, JS) uploads the code units as they are.  A surrogate pair becomes one
// 4-byte char, a lone surrogate (also: a pair cut by a document boundary) becomes EF BF BD, as GetBytes does.
//   k_u16_len     per 1024-unit tile (one wavefront, 16 units per lane): UTF-8 length of every unit -> tile sum and the
//                 exclusive prefix of every 16-unit group inside the tile
//   (scan of the tile sums: k_scan_*)
//   k_u16_write   the bytes, staged per tile in LDS and copied out coalesced; for the special entries' literal search (a registered literal holds U+FFFD) also
//                 the replaced-byte bitmap: one bit, over output bytes, at the EF of every U+FFFD that stands for a lone surrogate
//   k_u16_docoffs byte offset of every document = tile base + group prefix + the units of the group before it
// -------------------------------------------------------------------------------------------------
constexpr int kU16Tile = 1024;      // code units per wavefront
constexpr int kU16Lane = 16;        // ... per lane
// UTF-8 length of unit u at a position whose neighbours are prev/next (0 when there is none inside the document):
// 0 for the low half of a pair (its bytes belong to the high half)
TKZ_HD int tkz_u16_len(uint32_t u, uint32_t prev, bool has_prev, uint32_t next, bool has_next) {
    if (u < 0x80u) return 1;
    if (u < 0x800u) return 2;
    if (u - 0xD800u < 0x400u) return (has_next && next - 0xDC00u < 0x400u) ? 4 : 3;      // high surrogate: pair, or alone -> U+FFFD
    if (u - 0xDC00u < 0x400u) return (has_prev && prev - 0xD800u < 0x400u) ? 0 : 3;      // low surrogate: second half, or alone -> U+FFFD
    return 3;
}
TKZ_HD int tkz_u16_put(uint32_t u, uint32_t next, int len, uint8_t* o) {
    if (len == 1) { o[0] = (uint8_t)u; }
    else if (len == 2) { o[0] = (uint8_t)(0xC0u | (u >> 6)); o[1] = (uint8_t)(0x80u | (u & 0x3Fu)); }
    else if (len == 4) {
        const uint32_t c = 0x10000u + ((u - 0xD800u) << 10) + (next - 0xDC00u);
        o[0] = (uint8_t)(0xF0u | (c >> 18)); o[1] = (uint8_t)(0x80u | ((c >> 12) & 0x3Fu)); o[2] = (uint8_t)(0x80u | ((c >> 6) & 0x3Fu)); o[3] = (uint8_t)(0x80u | (c & 0x3Fu));
    } else if (len == 3) {
        const uint32_t c = (u - 0xD800u < 0x800u) ? 0xFFFDu : u;
        o[0] = (uint8_t)(0xE0u | (c >> 12)); o[1] = (uint8_t)(0x80u | ((c >> 6) & 0x3Fu)); o[2] = (uint8_t)(0x80u | (c & 0x3Fu));
    }
    return len;
}
// the units of this lane's group (and the one after it), its document-start bits, the lengths; returns the lane sum
struct TkzU16Lane { uint32_t u[kU16Lane + 1]; uint8_t len[kU16Lane]; };
TKZ_DEV int tkz_u16_lane(const uint16_t* units, int64_t total, const uint64_t* docbits, int64_t tile, TkzU16Lane* L) {
    const int lane = simt::lane();
    const int64_t p0 = tile * kU16Tile + (int64_t)lane * kU16Lane;
    uint32_t w[8];
    if (p0 + kU16Lane <= total) {
        const uint4 a = tkz_load16(units + p0), b = tkz_load16(units + p0 + 8);
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    } else {
        for (int k = 0; k < 8; ++k) {
            const int64_t q = p0 + 2 * k;
            w[k] = (q < total ? (uint32_t)units[q] : 0u) | ((q + 1 < total ? (uint32_t)units[q + 1] : 0u) << 16);
        }
    }
#pragma unroll
    for (int k = 0; k < kU16Lane; ++k) L->u[k] = (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
    // neighbours across the lane edge: the last unit of the lane below, the first unit of the lane above
    uint32_t prev = simt::shflu(L->u[kU16Lane - 1], (lane + 63) & 63), next = simt::shflu(L->u[0], (lane + 1) & 63);
    if (lane == 0) prev = p0 > 0 ? (uint32_t)units[p0 - 1] : 0u;
    if (lane == 63) next = p0 + kU16Lane < total ? (uint32_t)units[p0 + kU16Lane] : 0u;
    L->u[kU16Lane] = next;
    // document-start bits of positions p0 .. p0 + 16 (17 bits)
    const int64_t wd = p0 >> 6; const int sh = (int)(p0 & 63);
    uint64_t ds = p0 < total ? docbits[wd] >> sh : 0ull;                       // (docbits has total/64 + 1 words)
    if (sh == 48 && p0 + kU16Lane <= total) ds |= (docbits[wd + 1] & 1ull) << 16;
    int sum = 0;
#pragma unroll
    for (int k = 0; k < kU16Lane; ++k) {
        const int64_t q = p0 + k;
        int len = 0;
        if (q < total) {
            const bool has_prev = q > 0 && !((ds >> k) & 1ull);                 // not the first unit of its document
            const bool has_next = q + 1 < total && !((ds >> (k + 1)) & 1ull);   // not the last one
            len = tkz_u16_len(L->u[k], k ? L->u[k - 1] : prev, has_prev, L->u[k + 1], has_next);
        }
        L->len[k] = (uint8_t)len; sum += len;
    }
    return sum;
}
TKZ_KERNEL(256) void k_u16_len(const uint16_t* units, int64_t total, const uint64_t* docbits, int64_t ntiles, int32_t* grp_prefix, int32_t* tile_sum) {
    const int64_t tile = simt::bid() * (kThreads / 64) + simt::wave();
    if (tile >= ntiles) return;
    TkzU16Lane L;
    const int sum = tkz_u16_lane(units, total, docbits, tile, &L);
    int tot;
    const int pre = tkz_wave_scan_sum(sum, &tot);
    grp_prefix[tile * 64 + simt::lane()] = pre;
    if (simt::lane() == 0) tile_sum[tile] = tot;
}
TKZ_KERNEL(256) void k_u16_write(const uint16_t* units, int64_t total, const uint64_t* docbits, int64_t ntiles, const int64_t* tile_base,
                                 uint8_t* out, uint64_t* repl) {
    TKZ_SHARED uint8_t s_stage[kThreads / 64][3 * kU16Tile + 16];            // (a unit yields at most 3 bytes: a pair is 4 for 2 units)
    const int64_t tile = simt::bid() * (kThreads / 64) + simt::wave();
    if (tile >= ntiles) return;
    TkzU16Lane L;
    const int sum = tkz_u16_lane(units, total, docbits, tile, &L);
    int tot;
    int pos = tkz_wave_scan_sum(sum, &tot);
    uint8_t* st = s_stage[simt::wave()];
#pragma unroll
    for (int k = 0; k < kU16Lane; ++k) {
        // (lone surrogates are rare: an atomic each -- tiles, and lanes, share bitmap words)
        if (repl && L.len[k] == 3 && L.u[k] - 0xD800u < 0x800u) {
            const int64_t b = tile_base[tile] + pos;
            simt::atomic_or64((unsigned long long*)&repl[b >> 6], 1ull << (b & 63));
        }
        pos += tkz_u16_put(L.u[k], L.u[k + 1], L.len[k], st + pos);
    }
    (void)simt::ballot(true);          // (the staging area is private to the wavefront: its LDS accesses are ordered, no barrier)
    uint8_t* dst = out + tile_base[tile];
    for (int i = simt::lane(); i < tot; i += 64) dst[i] = st[i];
}
TKZ_KERNEL(256) void k_u16_docoffs(const uint16_t* units, int64_t total, const uint64_t* docbits, const int64_t* unit_offs, int64_t n_docs,
                                   const int64_t* tile_base, const int32_t* grp_prefix, const int64_t* grand, int64_t* byte_offs) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d <= n_docs; d += stride) {
        const int64_t p = unit_offs[d];
        if (p >= total) { byte_offs[d] = *grand; continue; }
        if (p < 0) { byte_offs[d] = 0; continue; }
        const int64_t g0 = p & ~(int64_t)(kU16Lane - 1);
        int64_t v = tile_base[p / kU16Tile] + grp_prefix[p / kU16Lane];
        for (int64_t q = g0; q < p; ++q) {                                 // the units of the group that belong to the document before
            const bool has_prev = q > 0 && !((docbits[q >> 6] >> (q & 63)) & 1ull);
            const bool has_next = q + 1 < total && !((docbits[(q + 1) >> 6] >> ((q + 1) & 63)) & 1ull);
            v += tkz_u16_len(units[q], q > 0 ? units[q - 1] : 0u, has_prev, q + 1 < total ? units[q + 1] : 0u, has_next);
        }
        byte_offs[d] = v;
    }
}

// -------------------------------------------------------------------------------------------------
// piece granularity (EncodeTrimSuffix / EncodeTrimPrefix walk the regex matches, TikTokenizer.cs:288-341, :483-519): the byte
// offset of every piece and the first piece of every document, straight from the piece-start bitmap -- no host round trip
//   (k_doccount2 + scan over STARTBITS give every sub-tile its first piece ordinal)
//   k_piece_index   one wavefront per sub-tile: positions of the set bits below `total`, in order
//   k_doc_piece     first piece of document d = number of piece starts before its first byte
// The encode kernels then run with the piece-start bitmap AS the document bitmap: they record the token position of every
// piece start, and k_docoffs over the piece offsets yields the token range of every piece in the same pass as the ids.
// -------------------------------------------------------------------------------------------------
TKZ_KERNEL(256) void k_piece_index(const uint64_t* startbits, int64_t nwords, int64_t total, int64_t nsub, const int64_t* ord_base,
                                   int64_t n_pieces, int64_t* piece_offs) {
    static_assert(kSub / 64 == 16, "one bitmap word per lane 0..15");
    const int lane = simt::lane();
    const int64_t sub = simt::bid() * (kThreads / 64) + simt::wave();
    if (sub == 0 && lane == 0) piece_offs[n_pieces] = total;
    if (sub >= nsub) return;
    const int64_t w = sub * (kSub / 64) + lane;
    uint64_t m = (lane < kSub / 64 && w < nwords) ? startbits[w] : 0ull;
    const int64_t lim = total - (w << 6);                 // bits at or beyond `total` (the sentinel) are not pieces
    if (lim <= 0) m = 0; else if (lim < 64) m &= tkz_lowmask((int)lim);
    int tot;
    const int pre = tkz_wave_scan<7>(tkz_popc64(m), &tot);
    int64_t o = ord_base[sub] + pre;
    for (; m; m &= m - 1) piece_offs[o++] = (w << 6) + tkz_ctz64(m);
}
TKZ_KERNEL(256) void k_doc_piece(const int64_t* offs, int64_t n_docs, int64_t total, const uint64_t* startbits, const int64_t* ord_base,
                                 int64_t n_pieces, int64_t* doc_piece) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d <= n_docs; d += stride) {
        const int64_t pos = offs[d];
        if (pos >= total) { doc_piece[d] = n_pieces; continue; }
        if (pos < 0) { doc_piece[d] = 0; continue; }
        const int64_t sub = pos / kSub, wpos = pos >> 6;
        int64_t ord = ord_base[sub];
        for (int64_t w = sub * (kSub / 64); w < wpos; ++w) ord += tkz_popc64(startbits[w]);
        ord += tkz_popc64(startbits[wpos] & tkz_lowmask((int)(pos & 63)));
        doc_piece[d] = ord;
    }
}

// -------------------------------------------------------------------------------------------------
// EncodeTrimSuffix / EncodeTrimPrefix for a batch (TikTokenizer.cs:288-579), behind the piece-granular launch sequence: the items of a document are its
// pieces (a taken special-token literal is ONE piece of ONE token: k_lit_fix, k_probe_special), piece_toffs their cumulative token counts.
//   k_trim_cut      one lane per document: the cut -- an item boundary, found by binary search over the document's range of piece_toffs --, the kept token
//                   range, the cut's byte position
//                     suffix: the longest run of leading items whose tokens sum to at most the maximum (every item has a token: the reference's loop, :296-340)
//                     prefix: everything when the document has at most the maximum; else the items up to the first boundary whose cumulative count reaches
//                             count - maximum go (TrimPrefix, :470-483)
//   (k_scan_partials64, k_scan_top, k_scan_final64: the kept lengths -> the kept ids' offsets.  k_scan_partials / k_scan_final with 64-bit counts: a
//    document of a batch beyond 2^31 bytes may keep more than 2^31 tokens)
//   k_trim_gather   the kept ids, compacted; the work is dealt out by OUTPUT position, a wavefront per kTrimTile ids (one long document beside thousands of
//                   short ones is so many tiles, not one lane's loop).  Then cut_units, dealt out by INPUT position: a wavefront per kTrimByteTile bytes of
//                   text counts the UTF-16 units (a unit per non-continuation byte, one more for a byte >= 0xF0) of what each of its documents has in front
//                   of its cut and adds them to the document's entry.
// An attempt whose counter block holds an error bit has offsets that mean nothing (records that did not fit, offsets that do not ascend ...): its result is
// thrown away by the host, and these kernels leave the caller's ids alone.
// -------------------------------------------------------------------------------------------------
constexpr int kTrimTile = 2048, kTrimByteTile = 4096;
TKZ_KERNEL(256) void k_trim_cut(TrimParams R) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    const bool bad = R.counters[0] != 0;
    for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d < R.n_docs; d += stride) {
        int64_t lo_t = 0, n_t = 0, cut = 0, a = 0;
        if (!bad) {
            a = R.offs[d];
            const int64_t b = R.offs[d + 1], p0 = R.doc_piece[d], p1 = R.doc_piece[d + 1];      // (an empty document: p0 == p1; the last one ends at `total`, piece n_pieces)
            const int64_t t0 = R.piece_toffs[p0], count = R.piece_toffs[p1] - t0;
            int64_t m = R.d_max ? R.d_max[d] : R.max_tokens;
            if (m < 0) m = 0;
            int64_t k = p0;                                      // the boundary of the cut: in front of piece k
            if (R.side == 0) {
                int64_t lo = p0, hi = p1;                        // the last boundary with at most m tokens in front of it (p0 has none)
                while (lo < hi) { const int64_t mid = lo + (hi - lo + 1) / 2; if (R.piece_toffs[mid] - t0 <= m) lo = mid; else hi = mid - 1; }
                k = lo; lo_t = t0; n_t = R.piece_toffs[k] - t0;
            } else {
                if (count > m) {
                    const int64_t need = count - m;              // the first boundary with at least `need` tokens in front of it (p1 has count)
                    int64_t lo = p0, hi = p1;
                    while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (R.piece_toffs[mid] - t0 >= need) hi = mid; else lo = mid + 1; }
                    k = lo;
                }
                lo_t = R.piece_toffs[k]; n_t = t0 + count - lo_t;
            }
            cut = k >= p1 ? b : (k == p0 ? a : R.piece_boffs[k]);
        }
        R.keep_lo[d] = lo_t; R.keep_n[d] = n_t > 0 ? n_t : 0; R.cut_pos[d] = cut;
        if (R.cut_bytes) R.cut_bytes[d] = cut - a;
        if (R.cut_units) R.cut_units[d] = 0;
    }
}
TKZ_DEV int64_t tkz_shfl64(int64_t v, int src) {
    const uint32_t lo = simt::shflu((uint32_t)v, src), hi = simt::shflu((uint32_t)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
TKZ_KERNEL(256) void k_scan_partials64(const int64_t* cnt, int64_t n, int64_t* bsum) {
    TKZ_SHARED int64_t s_w[4];
    const int64_t i0 = simt::bid() * kScanBlock;
    int64_t v = 0;
    for (int j = simt::tid(); j < kScanBlock; j += kThreads) if (i0 + j < n) v += cnt[i0 + j];
    for (int d = 32; d >= 1; d >>= 1) v += tkz_shfl64(v, simt::lane() ^ d);
    if (simt::lane() == 0) s_w[simt::wave()] = v;
    simt::sync();
    if (simt::tid() == 0) bsum[simt::bid()] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
TKZ_KERNEL(256) void k_scan_final64(const int64_t* cnt, int64_t n, const int64_t* boff, int64_t* base) {
    TKZ_SHARED int64_t s_w[kThreads / 64];
    const int lane = simt::lane(), wave = simt::wave();
    const int64_t i0 = simt::bid() * kScanBlock;
    constexpr int per = kScanBlock / kThreads;               // each thread owns `per` consecutive entries
    int64_t local[per], sum = 0;
    for (int j = 0; j < per; ++j) { const int64_t i = i0 + (int64_t)simt::tid() * per + j; local[j] = i < n ? cnt[i] : 0; sum += local[j]; }
    int64_t x = sum;                                         // inclusive scan inside the wavefront, then the wavefronts' totals
    for (int d = 1; d < 64; d <<= 1) { const int64_t y = tkz_shfl64(x, lane - d < 0 ? lane : lane - d); if (lane >= d) x += y; }
    if (lane == 63) s_w[wave] = x;
    simt::sync();
    int64_t run = boff[simt::bid()] + x - sum;
    for (int w = 0; w < wave; ++w) run += s_w[w];
    for (int j = 0; j < per; ++j) { const int64_t i = i0 + (int64_t)simt::tid() * per + j; if (i < n) base[i] = run; run += local[j]; }
}
// the last entry of the ascending offs[0 .. n] that is <= x (offs[0] <= x < offs[n]); entries that repeat -- empty documents -- give the last of them
TKZ_DEV int64_t tkz_last_le(const int64_t* offs, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) { const int64_t mid = lo + (hi - lo + 1) / 2; if (offs[mid] <= x) lo = mid; else hi = mid - 1; }
    return lo;
}
TKZ_KERNEL(256) void k_trim_gather(TrimParams R, const int32_t* ids, int64_t ids_cap, const int64_t* out_offs, int32_t* out, int64_t out_cap, int64_t* kept_total) {
    const int lane = simt::lane();
    const int64_t nwaves = simt::nblocks() * (kThreads / 64), wave0 = simt::bid() * (kThreads / 64) + simt::wave();
    const int64_t kept = out_offs[R.n_docs];
    if (wave0 == 0 && lane == 0) *kept_total = kept;
    if (R.counters[0] != 0 || kept < 0) return;
    if (kept <= out_cap) {
        const int64_t ntile = (kept + kTrimTile - 1) / kTrimTile;
        for (int64_t t = wave0; t < ntile; t += nwaves) {
            const int64_t q0 = t * kTrimTile, q1 = q0 + kTrimTile < kept ? q0 + kTrimTile : kept;
            const int64_t d0 = tkz_last_le(out_offs, 0, R.n_docs - 1, q0), d1 = tkz_last_le(out_offs, d0, R.n_docs - 1, q1 - 1);     // (wave-uniform)
            const int64_t shift0 = R.keep_lo[d0] - out_offs[d0];
            for (int64_t q = q0 + lane; q < q1; q += 64) {
                // a tile inside one document is a straight copy; else every lane finds the document of its id among the tile's
                int64_t s = shift0 + q;
                if (d0 != d1) { const int64_t d = tkz_last_le(out_offs, d0, d1, q); s = R.keep_lo[d] + (q - out_offs[d]); }
                if (s >= 0 && s < ids_cap) tkz_store_nt(out + q, tkz_load_nt(ids + s));
            }
        }
    }
    if (!R.cut_units) return;
    const int64_t nbt = (R.total + kTrimByteTile - 1) / kTrimByteTile;
    for (int64_t t = wave0; t < nbt; t += nwaves) {
        const int64_t b0 = t * kTrimByteTile, b1 = b0 + kTrimByteTile < R.total ? b0 + kTrimByteTile : R.total;
        // the documents with bytes in [b0, b1), 64 at a time: a lane reads one document's range, the wavefront then counts the ranges that are not empty one by one
        const int64_t d0 = tkz_last_le(R.offs, 0, R.n_docs - 1, b0), d1 = tkz_last_le(R.offs, d0, R.n_docs - 1, b1 - 1);
        for (int64_t dc = d0; dc <= d1; dc += 64) {
            const int64_t d = dc + lane;
            int64_t lo = 0, hi = 0;
            if (d <= d1) { lo = R.offs[d]; hi = R.cut_pos[d]; if (lo < b0) lo = b0; if (hi > b1) hi = b1; }
            for (uint64_t m = simt::ballot(lo < hi); m; m &= m - 1) {
                const int src = tkz_ctz64(m);
                const int64_t rlo = tkz_shfl64(lo, src), rhi = tkz_shfl64(hi, src);
                int c = 0;
                for (int64_t i = rlo + lane; i < rhi; i += 64) { const uint32_t x = R.bytes[i]; c += ((x & 0xC0u) != 0x80u ? 1 : 0) + (x >= 0xF0u ? 1 : 0); }
                int tot;
                (void)tkz_wave_scan_sum(c, &tot);
                if (lane == 0 && tot) simt::atomic_add64(reinterpret_cast<unsigned long long*>(R.cut_units + dc + src), (unsigned long long)tot);
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------
// Packed rows (tkz_encode_batch_packed_device; tkz.h states the rule), behind the plain document-granular launch sequence.  The stream is every document's
// [bos] ids [eos]; document d starts at s[d] = O[d] + f * d (O: the unframed offsets, f: 0, 1 or 2 framing ids a document), never stored: the searches compute
// it from O.  The work is dealt out by OUTPUT position as k_trim_gather deals it: a wavefront per tile of kPackTile stream positions, grid-strided.
//   k_pack_count   the segment starts of every tile (a position whose pos is 0)
//   (k_scan_partials, k_scan_top, k_scan_final: the counts -> the rank of every tile's first segment start, and n_segs)
//   k_pack_write   the framed ids (f > 0; with f == 0 k_place wrote them where they stand), the pad tail, pos, seg_starts in ascending order, the framed offsets
// Both are ONE body (tkz_pack_tiles<WRITE>), so the count and the write cannot disagree about the predicate.  The position inside the row costs one 64-bit
// remainder a TILE (wave-uniform); a lane then steps it by 64 with one conditional subtraction.  With f == 0 a run of empty documents repeats an offset and the
// search returns the last of them -- the document that holds the position; an empty document starts no segment there.
// -------------------------------------------------------------------------------------------------
// the last d of [lo, hi] with s[d] <= x (s[lo] <= x)
TKZ_DEV int64_t tkz_pack_doc(const int64_t* offs, int64_t f, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) { const int64_t mid = lo + (hi - lo + 1) / 2; if (offs[mid] + f * mid <= x) lo = mid; else hi = mid - 1; }
    return lo;
}
template <bool WRITE> TKZ_DEV void tkz_pack_tiles(const PackParams& K) {
    const int lane = simt::lane();
    const int64_t nwaves = simt::nblocks() * (kThreads / 64), wave0 = simt::bid() * (kThreads / 64) + simt::wave();
    const int64_t fb = K.bos_id >= 0 ? 1 : 0, fe = K.eos_id >= 0 ? 1 : 0, f = fb + fe, L = K.row_len;
    const bool bad = K.counters[0] != 0;
    const int64_t T = bad ? 0 : *K.grand + f * K.n_docs;
    const int64_t n_rows = (T + L - 1) / L, full = n_rows * L;
    if (!WRITE) {
        if (wave0 == 0 && lane == 0) { K.totals[0] = T; K.totals[1] = n_rows; }
    } else {
        if (bad) return;                                       // (a failed attempt: the offsets mean nothing, the caller's buffers are left alone)
        if (f > 0) {                                           // (a lane a document; O is the workspace's, so no reader of it is overtaken)
            const int64_t stride = simt::nblocks() * simt::nthreads();
            for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d <= K.n_docs; d += stride) K.out_offs[d] = K.offs[d] + f * d;
        }
        const int64_t n_segs = K.totals[2];
        if (full > K.out_cap || (K.seg_starts && n_segs > K.seg_cap)) return;
        if (K.seg_starts && wave0 == 0 && lane == 0) K.seg_starts[n_segs] = T;
    }
    const int64_t ntile = WRITE ? (full + kPackTile - 1) / kPackTile : K.ntile;
    const bool pad_only = WRITE && f == 0 && !K.pos && !K.seg_starts;      // (the ids stand where k_place wrote them: only the tail is left to write)
    for (int64_t t = wave0; t < ntile; t += nwaves) {
        const int64_t q0 = t * kPackTile;
        if (pad_only && q0 + kPackTile <= T) continue;
        const int64_t q1 = WRITE ? (q0 + kPackTile < full ? q0 + kPackTile : full) : q0 + kPackTile;
        const int64_t qT = q1 < T ? q1 : T;                    // the stream's part of the tile: [q0, qT)
        // the two documents at its ends (wave-uniform); a tile inside one document needs no search by the lanes
        int64_t d0 = 0, d1 = 0, od = 0, sd = 0, se = 0;
        if (q0 < qT) {
            // (a framed document holds a position at least: the tile's last document is then fewer than kPackTile documents on)
            d0 = tkz_pack_doc(K.offs, f, 0, K.n_docs - 1, q0);
            const int64_t dmax = f > 0 && d0 + kPackTile < K.n_docs ? d0 + kPackTile - 1 : K.n_docs - 1;
            d1 = tkz_pack_doc(K.offs, f, d0, dmax, qT - 1);
            od = K.offs[d0]; sd = od + f * d0; se = K.offs[d0 + 1] + f * (d0 + 1);
        }
        // the position inside the row: q0's by one division, the lane's and every later one's by additions (m < L and step < L: one subtraction is enough)
        const int64_t m0 = q0 % L;
        int64_t m, step;
        if (L >= kPackTile) { m = m0 + lane; if (m >= L) m -= L; step = 64; }
        else { m = (int64_t)(((uint32_t)m0 + (uint32_t)lane) % (uint32_t)L); step = (int64_t)(64u % (uint32_t)L); }
        const int64_t base = WRITE && K.seg_starts && t < K.ntile ? K.base[t] : 0;
        int run = 0;                                           // the tile's segment starts in front of this group of 64 positions
        int64_t dl = d0, o = od, s = sd, e = se;               // the lane's document: its positions ascend, so the search goes on from the last one's
        for (int64_t g = q0; g < q1; g += 64) {
            const int64_t q = g + lane;
            bool seg = false;
            if (q < qT) {
                if (q >= e) { dl = tkz_pack_doc(K.offs, f, dl, d1, q); o = K.offs[dl]; s = o + f * dl; e = K.offs[dl + 1] + f * (dl + 1); }
                const int64_t j = q - s, p = j < m ? j : m;    // behind the document's start, behind the row's: pos is the nearer of the two
                seg = p == 0;
                if (WRITE) {
                    if (f > 0) {
                        int32_t v = K.pad_id;
                        const int64_t src = o + j - fb;
                        if (fb && j == 0) v = K.bos_id;
                        else if (fe && q == e - 1) v = K.eos_id;
                        else if (src >= 0 && src < K.ids_cap) v = tkz_load_nt(K.ids + src);
                        tkz_store_nt(K.out + q, v);
                    }
                    if (K.pos) tkz_store_nt(K.pos + q, (int32_t)p);
                }
            } else if (WRITE && q < q1) {                      // the pad tail
                tkz_store_nt(K.out + q, K.pad_id);
                if (K.pos) tkz_store_nt(K.pos + q, 0);
            }
            const uint64_t mask = simt::ballot(seg);
            if (WRITE && K.seg_starts && seg) K.seg_starts[base + run + tkz_popc64(mask & tkz_lowmask(lane))] = q;
            run += tkz_popc64(mask);
            m += step; if (m >= L) m -= L;
        }
        if (!WRITE && lane == 0) K.cnt[t] = run;
    }
}
TKZ_KERNEL(256) void k_pack_count(PackParams K) { tkz_pack_tiles<false>(K); }
TKZ_KERNEL(256) void k_pack_write(PackParams K) { tkz_pack_tiles<true>(K); }

// -------------------------------------------------------------------------------------------------
// Decode for a batch (TikTokenizer.Decode, TikTokenizer.cs:586-604): id -> bytes through the decoder table, ids that are in
// neither the vocabulary nor the registered special tokens contribute nothing (:591-599), documents concatenated.
//   k_dec_len      per 1024-id tile (one wavefront, 16 ids per lane): byte length of every id -> tile sum and the exclusive
//                  prefix of every 16-id group inside the tile
//   (scan of the tile sums: k_scan_*)
//   k_dec_write    the bytes, staged per tile in LDS and copied out coalesced (direct copies when a tile exceeds the stage)
//   k_dec_docoffs  byte offset of every document = tile base + group prefix + the ids of the group before it
// -------------------------------------------------------------------------------------------------
constexpr int kDecTile = 1024, kDecLane = 16, kDecStage = 12288;
TKZ_DEV bool tkz_dec_find(const TkzDecodeTable& D, int32_t id, uint32_t* off, uint32_t* len) {
    int64_t k;
    if (D.dense) { if (id < 0 || (int64_t)id >= D.n) return false; k = id; }
    else {
        int64_t lo = 0, hi = D.n;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (D.ids[mid] < id) lo = mid + 1; else hi = mid; }
        if (lo >= D.n || D.ids[lo] != id) return false;
        k = lo;
    }
    *off = D.off[k]; *len = D.off[k + 1] - D.off[k];
    return *len != 0;
}
struct TkzDecLane { uint32_t off[kDecLane]; uint32_t len[kDecLane]; };
TKZ_DEV int tkz_dec_lane(const TkzDecodeTable& D, const int32_t* ids, int64_t total, int64_t tile, TkzDecLane* L) {
    const int64_t p0 = tile * kDecTile + (int64_t)simt::lane() * kDecLane;
    int sum = 0;
#pragma unroll
    for (int k = 0; k < kDecLane; ++k) {
        L->off[k] = 0; L->len[k] = 0;
        if (p0 + k < total) { uint32_t o, n; if (tkz_dec_find(D, ids[p0 + k], &o, &n)) { L->off[k] = o; L->len[k] = n; } }
        sum += (int)L->len[k];
    }
    return sum;
}
TKZ_KERNEL(256) void k_dec_len(TkzDecodeTable D, const int32_t* ids, int64_t total, int64_t ntiles, int32_t* grp_prefix, int32_t* tile_sum) {
    const int64_t tile = simt::bid() * (kThreads / 64) + simt::wave();
    if (tile >= ntiles) return;
    TkzDecLane L;
    const int sum = tkz_dec_lane(D, ids, total, tile, &L);
    int tot;
    const int pre = tkz_wave_scan_sum(sum, &tot);
    grp_prefix[tile * 64 + simt::lane()] = pre;
    if (simt::lane() == 0) tile_sum[tile] = tot;
}
TKZ_KERNEL(256) void k_dec_write(TkzDecodeTable D, const int32_t* ids, int64_t total, int64_t ntiles, const int64_t* tile_base, uint8_t* out, int64_t out_cap) {
    TKZ_SHARED uint8_t s_stage[kThreads / 64][kDecStage];
    const int64_t tile = simt::bid() * (kThreads / 64) + simt::wave();
    if (tile >= ntiles) return;
    TkzDecLane L;
    const int sum = tkz_dec_lane(D, ids, total, tile, &L);
    int tot;
    int pos = tkz_wave_scan_sum(sum, &tot);
    const int64_t base = tile_base[tile];
    if (base + tot > out_cap) return;                       // (the host reports TKZ_E_CAPACITY from the grand total)
    uint8_t* dst = out + base;
    if (tot <= kDecStage) {
        uint8_t* st = s_stage[simt::wave()];
#pragma unroll 1
        for (int k = 0; k < kDecLane; ++k) { const uint8_t* src = D.blob + L.off[k]; for (uint32_t j = 0; j < L.len[k]; ++j) st[pos + (int)j] = src[j]; pos += (int)L.len[k]; }
        (void)simt::ballot(true);      // (the staging area is private to the wavefront: its LDS accesses are ordered, no barrier)
        for (int i = simt::lane(); i < tot; i += 64) dst[i] = st[i];
    } else {
#pragma unroll 1
        for (int k = 0; k < kDecLane; ++k) { const uint8_t* src = D.blob + L.off[k]; for (uint32_t j = 0; j < L.len[k]; ++j) dst[pos + (int)j] = src[j]; pos += (int)L.len[k]; }
    }
}
TKZ_KERNEL(256) void k_dec_docoffs(TkzDecodeTable D, const int32_t* ids, int64_t total, const int64_t* id_offs, int64_t n_docs, const int64_t* tile_base,
                                   const int32_t* grp_prefix, const int64_t* grand, int64_t* byte_offs, int32_t* counters) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d <= n_docs; d += stride) {
        const int64_t p = id_offs[d];
        bool ok = p >= 0 && p <= total;
        if (d == 0) ok = ok && p == 0;
        if (d == n_docs) ok = ok && p == total; else ok = ok && p <= id_offs[d + 1];
        if (!ok) { simt::atomic_or((unsigned*)&counters[0], (unsigned)kErrOffsets); byte_offs[d] = 0; continue; }
        if (p >= total) { byte_offs[d] = *grand; continue; }
        int64_t v = tile_base[p / kDecTile] + grp_prefix[p / kDecLane];
        for (int64_t q = p & ~(int64_t)(kDecLane - 1); q < p; ++q) { uint32_t o, n; if (tkz_dec_find(D, ids[q], &o, &n)) v += n; }
        byte_offs[d] = v;
    }
}

// -------------------------------------------------------------------------------------------------
// Decoded documents -> UTF-16 documents on the device (the batch form of Encoding.UTF8.GetString, TikTokenizer.cs:603; WHATWG
// TextDecoder("utf-8") in the TypeScript reference): the mirror of the k_u16_* family.  The bytes of k_dec_write are routinely
// not well-formed -- keys are byte fragments, a trimmed id list ends inside a char --, and both references replace every
// MAXIMAL SUBPART of an ill-formed sequence (Unicode 3.9, table 3-7) by one U+FFFD.  An ITEM is a well-formed char or such a
// subpart.  Whether a byte starts an item is decidable from the 3 bytes before it: a lead byte or a byte that can start nothing
// always does; a continuation byte does not iff the first non-continuation byte up to 3 bytes back INSIDE ITS DOCUMENT is a
// lead that accepts every byte up to and including this one.  A lead looks at most 3 bytes ahead, inside its document, to
// see whether its sequence completes (a char: one unit, or a pair for 4 bytes) or not (its accepted prefix: one U+FFFD).
//   k_u8_len      per 1024-byte tile (one wavefront, 16 bytes per lane): units of every byte -> tile sum and the exclusive
//                 prefix of every 16-byte group inside the tile
//   (scan of the tile sums: k_scan_*)
//   k_u8_write    the units, staged per tile in LDS and copied out coalesced
//   k_u8_docoffs  unit offset of every document = tile base + group prefix + the bytes of the group before it
// -------------------------------------------------------------------------------------------------
constexpr int kU8Tile = 1024;       // bytes per wavefront
constexpr int kU8Lane = 16;         // ... per lane
constexpr int kU8Stage = kU8Tile + 8;   // units a tile can yield: a byte each, and one more for a 4-byte lead in its last byte (whose pair is 2 units: the rest of it lies in the next tile)
// continuation bytes a lead asks for (0: no lead -- ASCII, a continuation byte, C0, C1, F5..FF)
TKZ_HD int tkz_u8_need(uint32_t b) { return b - 0xC2u < 0x1Eu ? 1 : (b - 0xE0u < 0x10u ? 2 : (b - 0xF0u < 5u ? 3 : 0)); }
TKZ_HD bool tkz_u8_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }
// table 3-7: the second byte a lead accepts (the third and fourth: any continuation byte)
TKZ_HD bool tkz_u8_second(uint32_t lead, uint32_t c) {
    const uint32_t lo = lead == 0xE0u ? 0xA0u : (lead == 0xF0u ? 0x90u : 0x80u), hi = lead == 0xEDu ? 0x9Fu : (lead == 0xF4u ? 0x8Fu : 0xBFu);
    return c >= lo && c <= hi;
}
// The units of byte b0 at a position q whose neighbours are p3 p2 p1 (q - 3 .. q - 1) and n1 n2 n3 (q + 1 .. q + 3).  ds: the document-start bits of
// q - 2 .. q + 3 (bit 2 = q itself): a neighbour counts only when no document starts between it and q.  Returns 0 (the byte belongs to the item a lead before
// it starts), 1 (*u0) or 2 (*u0, *u1: a pair).
TKZ_HD int tkz_u8_item(uint32_t p3, uint32_t p2, uint32_t p1, uint32_t b0, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t ds, uint32_t* u0, uint32_t* u1) {
    *u0 = 0xFFFDu; *u1 = 0u;
    if (b0 < 0x80u) { *u0 = b0; return 1; }
    if (tkz_u8_cont(b0)) {
        const bool back1 = !(ds & 4u), back2 = back1 && !(ds & 2u), back3 = back2 && !(ds & 1u);
        if (!back1) return 1;
        if (!tkz_u8_cont(p1)) return tkz_u8_need(p1) >= 1 && tkz_u8_second(p1, b0) ? 0 : 1;
        if (!back2) return 1;
        if (!tkz_u8_cont(p2)) return tkz_u8_need(p2) >= 2 && tkz_u8_second(p2, p1) ? 0 : 1;
        if (!back3) return 1;
        return tkz_u8_need(p3) == 3 && tkz_u8_second(p3, p2) ? 0 : 1;
    }
    const int need = tkz_u8_need(b0);
    if (need == 0) return 1;                                               // C0, C1, F5..FF
    const bool fwd1 = !(ds & 8u), fwd2 = fwd1 && !(ds & 16u), fwd3 = fwd2 && !(ds & 32u);
    if (!(fwd1 && tkz_u8_second(b0, n1))) return 1;
    if (need == 1) { *u0 = ((b0 & 0x1Fu) << 6) | (n1 & 0x3Fu); return 1; }
    if (!(fwd2 && tkz_u8_cont(n2))) return 1;
    if (need == 2) { *u0 = ((b0 & 0x0Fu) << 12) | ((n1 & 0x3Fu) << 6) | (n2 & 0x3Fu); return 1; }
    if (!(fwd3 && tkz_u8_cont(n3))) return 1;
    const uint32_t c = (((b0 & 0x07u) << 18) | ((n1 & 0x3Fu) << 12) | ((n2 & 0x3Fu) << 6) | (n3 & 0x3Fu)) - 0x10000u;
    *u0 = 0xD800u + (c >> 10); *u1 = 0xDC00u + (c & 0x3FFu);
    return 2;
}
// the document-start bits of positions q0 - 2 .. q0 + 29 (bit j = position q0 - 2 + j), q0 >= 0; docbits has nwords words
TKZ_HD uint32_t tkz_u8_bits(const uint64_t* docbits, int64_t nwords, int64_t q0) {
    if (q0 < 2) return (uint32_t)(docbits[0] << (2 - q0));
    const int64_t s = q0 - 2, wd = s >> 6; const int sh = (int)(s & 63);
    uint64_t v = wd < nwords ? docbits[wd] >> sh : 0ull;
    if (sh > 32 && wd + 1 < nwords) v |= docbits[wd + 1] << (64 - sh);
    return (uint32_t)v;
}
// the bytes of this lane's group with the 3 either side of it (b[3] is the group's first), its document-start bits (tkz_u8_bits of the group's
// first position: 21 are used); returns the lane sum
struct TkzU8Lane { uint32_t b[kU8Lane + 6]; uint32_t ds; };
TKZ_DEV int tkz_u8_lane(const uint8_t* bytes, int64_t total, const uint64_t* docbits, int64_t nwords, int64_t tile, TkzU8Lane* L) {
    const int lane = simt::lane();
    const int64_t p0 = tile * kU8Tile + (int64_t)lane * kU8Lane;
    uint32_t w[4];
    if (p0 + kU8Lane <= total) { const uint4 a = tkz_load16(bytes + p0); w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; }
    else {
        for (int k = 0; k < 4; ++k) {
            w[k] = 0u;
            for (int j = 0; j < 4; ++j) { const int64_t q = p0 + 4 * k + j; if (q < total) w[k] |= (uint32_t)bytes[q] << (8 * j); }
        }
    }
#pragma unroll
    for (int k = 0; k < kU8Lane; ++k) L->b[3 + k] = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    // neighbours across the lane edge: the last 3 bytes of the lane below, the first 3 of the lane above
    uint32_t prev = simt::shflu(w[3], (lane + 63) & 63) >> 8, next = simt::shflu(w[0], (lane + 1) & 63) & 0xFFFFFFu;
    if (lane == 0) { prev = 0u; for (int j = 1; j <= 3; ++j) if (p0 - j >= 0 && p0 - j < total) prev |= (uint32_t)bytes[p0 - j] << (8 * (3 - j)); }
    if (lane == 63) { next = 0u; for (int j = 0; j < 3; ++j) if (p0 + kU8Lane + j < total) next |= (uint32_t)bytes[p0 + kU8Lane + j] << (8 * j); }
#pragma unroll
    for (int j = 0; j < 3; ++j) { L->b[j] = (prev >> (8 * j)) & 0xFFu; L->b[3 + kU8Lane + j] = (next >> (8 * j)) & 0xFFu; }
    L->ds = p0 < total ? tkz_u8_bits(docbits, nwords, p0) : 0u;
    int sum = 0;
#pragma unroll
    for (int k = 0; k < kU8Lane; ++k) {
        uint32_t u0, u1;
        if (p0 + k < total) sum += tkz_u8_item(L->b[k], L->b[k + 1], L->b[k + 2], L->b[k + 3], L->b[k + 4], L->b[k + 5], L->b[k + 6], L->ds >> k, &u0, &u1);
    }
    return sum;
}
TKZ_KERNEL(256) void k_u8_len(const uint8_t* bytes, int64_t total, const uint64_t* docbits, int64_t nwords, int64_t ntiles, int32_t* grp_prefix, int32_t* tile_sum) {
    const int64_t tile = simt::bid() * (kThreads / 64) + simt::wave();
    if (tile >= ntiles) return;
    TkzU8Lane L;
    const int sum = tkz_u8_lane(bytes, total, docbits, nwords, tile, &L);
    int tot;
    const int pre = tkz_wave_scan_sum(sum, &tot);
    grp_prefix[tile * 64 + simt::lane()] = pre;
    if (simt::lane() == 0) tile_sum[tile] = tot;
}
// the units of this lane's group into the wavefront's stage, from `pos` -- the lane's exclusive prefix -- on (k_u8_write, k_dec_small)
TKZ_DEV void tkz_u8_stage(const TkzU8Lane& L, int64_t total, int64_t tile, int pos, uint16_t* st) {
    const int64_t p0 = tile * kU8Tile + (int64_t)simt::lane() * kU8Lane;
#pragma unroll
    for (int k = 0; k < kU8Lane; ++k) {
        uint32_t u0, u1;
        if (p0 + k < total) {
            const int n = tkz_u8_item(L.b[k], L.b[k + 1], L.b[k + 2], L.b[k + 3], L.b[k + 4], L.b[k + 5], L.b[k + 6], L.ds >> k, &u0, &u1);
            if (n >= 1) st[pos] = (uint16_t)u0;
            if (n == 2) st[pos + 1] = (uint16_t)u1;
            pos += n;
        }
    }
}
TKZ_KERNEL(256) void k_u8_write(const uint8_t* bytes, int64_t total, const uint64_t* docbits, int64_t nwords, int64_t ntiles, const int64_t* tile_base,
                                uint16_t* out, int64_t out_cap) {
    TKZ_SHARED uint16_t s_stage[kThreads / 64][kU8Stage];
    const int64_t tile = simt::bid() * (kThreads / 64) + simt::wave();
    if (tile >= ntiles) return;
    TkzU8Lane L;
    const int sum = tkz_u8_lane(bytes, total, docbits, nwords, tile, &L);
    int tot;
    int pos = tkz_wave_scan_sum(sum, &tot);
    const int64_t base = tile_base[tile];
    if (base + tot > out_cap || tot > kU8Stage) return;      // (the host reports TKZ_E_CAPACITY from the grand total)
    uint16_t* st = s_stage[simt::wave()];
    tkz_u8_stage(L, total, tile, pos, st);
    (void)simt::ballot(true);          // (the staging area is private to the wavefront: its LDS accesses are ordered, no barrier)
    uint16_t* dst = out + base;
    for (int i = simt::lane(); i < tot; i += 64) dst[i] = st[i];
}
// the units of the byte at q, its neighbours and bits read one by one (k_u8_docoffs: the few bytes between a group's start and a document's)
TKZ_DEV int tkz_u8_units_at(const uint8_t* bytes, int64_t total, const uint64_t* docbits, int64_t nwords, int64_t q) {
    uint32_t b[7], u0, u1;
    for (int j = 0; j < 7; ++j) { const int64_t r = q - 3 + j; b[j] = r >= 0 && r < total ? (uint32_t)bytes[r] : 0u; }
    return tkz_u8_item(b[0], b[1], b[2], b[3], b[4], b[5], b[6], tkz_u8_bits(docbits, nwords, q), &u0, &u1);
}
TKZ_KERNEL(256) void k_u8_docoffs(const uint8_t* bytes, int64_t total, const uint64_t* docbits, int64_t nwords, const int64_t* byte_offs, int64_t n_docs,
                                  const int64_t* tile_base, const int32_t* grp_prefix, const int64_t* grand, int64_t* unit_offs) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d <= n_docs; d += stride) {
        const int64_t p = byte_offs[d];
        if (p >= total) { unit_offs[d] = *grand; continue; }
        if (p < 0) { unit_offs[d] = 0; continue; }
        int64_t v = tile_base[p / kU8Tile] + grp_prefix[p / kU8Lane];
        for (int64_t q = p & ~(int64_t)(kU8Lane - 1); q < p; ++q) v += tkz_u8_units_at(bytes, total, docbits, nwords, q);      // the bytes of the group that belong to the document before
        unit_offs[d] = v;
    }
}

// -------------------------------------------------------------------------------------------------
// synthetic corpus (tkz_corpus.h): lengths, then bytes
// -------------------------------------------------------------------------------------------------
TKZ_KERNEL(256) void k_corpus_lengths(int kind, uint64_t seed, int64_t first_doc, int64_t n_docs, int min_len, int max_len, int64_t* offs) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d < n_docs; d += stride)
        offs[d + 1] = tkz_corpus_doc(kind, seed, first_doc + d, min_len, max_len, (uint8_t*)0, 0);
    if (simt::bid() == 0 && simt::tid() == 0) offs[0] = 0;
}
TKZ_KERNEL(256) void k_corpus_fill(int kind, uint64_t seed, int64_t first_doc, int64_t n_docs, int min_len, int max_len,
                                   const int64_t* offs, uint8_t* bytes, int64_t cap) {
    const int64_t stride = simt::nblocks() * simt::nthreads();
    for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d < n_docs; d += stride) {
        const int64_t a = offs[d], b = offs[d + 1];
        if (b <= cap) tkz_corpus_doc(kind, seed, first_doc + d, min_len, max_len, bytes + a, b - a);
    }
}
// in-place inclusive scan of offs[1..n] by one workgroup (lengths -> offsets); n up to 10^8 is ~100 ms, one-off setup
TKZ_KERNEL(256) void k_offsets_scan(int64_t* offs, int64_t n, int64_t* total) {
    TKZ_SHARED int64_t s_part[kThreads];
    const int tid = simt::tid();
    const int64_t per = (n + kThreads - 1) / kThreads;
    const int64_t lo = 1 + tid * per, hi = lo + per < n + 1 ? lo + per : n + 1;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += offs[i];
    s_part[tid] = s;
    simt::sync();
    int64_t run = 0;
    for (int t = 0; t < tid; ++t) run += s_part[t];
    for (int64_t i = lo; i < hi; ++i) { run += offs[i]; offs[i] = run; }
    simt::sync();
    if (tid == 0) *total = n ? offs[n] : 0;
}

// -------------------------------------------------------------------------------------------------
// Token-budget chunks (tkz_encode_batch_chunks_device), behind the piece-granular launch sequence -- which leaves the ids in the caller's buffer and the byte and
// token offset of every item (piece_boffs, piece_toffs: a taken special-token literal is ONE item of ONE token) and the first item of every document in the
// workspace.  The rule (tkz.h): a chunk that starts at token s ends at the largest item boundary b with s < b <= s + max; with none, at s + max inside the item.
// How many chunks there are is known only after the walk, so the documents are walked TWICE -- count, scan, write -- rather than written into slots reserved by the
// bound 2 * count / max + 1 and compacted: the walk reads piece_toffs only, a document that fits the budget costs two loads in either pass, and the table goes
// straight into the caller's arrays with nothing between to size, zero or move.
//   k_chunk_walk       one lane per document, the same kernel for both passes.  A document of at most max tokens is one chunk with no search.  Otherwise the end
//                      of a chunk is found by a galloping search forward from its start (1, 2, 4 ... items ahead, then a binary search inside the last stride):
//                      chunks span a few hundred items at most.  A document of more than kChunkLongItems items is put on a list instead.
//   k_chunk_walk_long  one wavefront per listed document: the lanes hold 64 consecutive piece_toffs entries (one coalesced load), a ballot of
//                      toffs <= s + max and a population count give the chunk's end; the window moves on only when a chunk runs past it, so a load
//                      serves every chunk that ends inside it, and the next three windows are loaded ahead.  What remains serial is one document's chain of chunks on ONE wavefront: a step a chunk, and
//                      a load per 64 items.
//   (k_scan_partials64, k_scan_top, k_scan_final64: the counts -> doc_chunk_offs)
//   the writing pass   chunk_tokens[c] = s (piece_toffs are batch-wide).  The byte start at an item boundary is piece_boffs; inside an item the walking lane adds
//                      the key lengths of the item's ids in front of s through the decode table (as k_tokspan_mark does), going on from where the chunk before
//                      stopped.  chunk_units[c] receives the BATCH byte position for k_chunk_units.
//   k_chunk_unitcount  the UTF-16 units begun in every span of kChunkUnitSpan = 128 bytes (tkz_span_units16 holds the rule); launch_scan: their exclusive scan.
//                      (Per 1 KiB sub-tile, as the span entries count, a chunk's position cost half a KiB of text read on average: 11 GB for the 24 million
//                      chunks of the headline batch at a budget of 64, and k_chunk_units was 8 - 10 ms of the call.)
//   k_chunk_units      a wavefront per 64 chunks, a lane finds the document of its chunk; for every chunk that is not its document's first a group of 16 lanes
//                      counts the units of the span in front of the position (8 lanes) and in front of the document's start (8 lanes): base + count, one
//                      minus the other.
// With an error bit in the counter block the counts are 0; with one, with ids that did not fit or with more chunks than chunk_cap the table is left alone.
// -------------------------------------------------------------------------------------------------
TKZ_DEV void tkz_span_units16(const uint8_t* bytes, int64_t total, int64_t p0, int64_t end, uint32_t* begun, uint32_t* four);      // (the span helpers, below)
TKZ_DEV int tkz_chunk_popc2(uint32_t a, uint32_t b) { return tkz_popc32(a) + tkz_popc32(b); }
// The end of the chunk that starts at token s inside item *p (toffs[*p] == *tp <= s < toffs[*p + 1]) of a document whose items end at p1, with MORE than m tokens
// left (toffs[p1] > s + m): the last item boundary at or below s + m -- *p and *tp move there -- or, when that is *p itself, s + m inside the item.
TKZ_DEV int64_t tkz_chunk_end(const int64_t* toffs, int64_t p1, int64_t s, int64_t m, int64_t* p, int64_t* tp) {
    const int64_t lim = s + m;
    int64_t lo = *p, tlo = *tp, hi = p1;
    for (int64_t step = 1; lo + step < hi; step <<= 1) {
        const int64_t i = lo + step, v = toffs[i];
        if (v > lim) { hi = i; break; }
        lo = i; tlo = v;
    }
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2, v = toffs[mid];
        if (v <= lim) { lo = mid; tlo = v; } else hi = mid;
    }
    if (lo == *p) return lim;
    *p = lo; *tp = tlo;
    return tlo;
}
struct TkzChunkItem { int64_t item, tok, pos; };           // the item a walk is inside of: its ids in front of token `tok` end at batch byte `pos`
// chunk o of the table: it starts at token s, in item p (whose first token is tp) of the document that starts at byte a; first: the document's first chunk
TKZ_DEV void tkz_chunk_emit(const ChunkParams& C, const TkzDecodeTable& D, int64_t o, int64_t a, bool first, int64_t s, int64_t p, int64_t tp, TkzChunkItem* W) {
    if (o < 0 || o >= C.chunk_cap) return;
    C.chunk_tokens[o] = s;
    if (!C.chunk_bytes && !C.chunk_units) return;
    int64_t pos = a;
    if (!first && s == tp) pos = C.piece_boffs[p];
    else if (!first) {
        const int64_t b0 = C.piece_boffs[p], b1 = C.piece_boffs[p + 1];
        if (W->item != p) { W->item = p; W->tok = tp; W->pos = b0; }
        bool bad = false;
        for (int64_t t = W->tok; t < s; ++t) {
            uint32_t off, len = 0;
            if (!tkz_dec_find(D, C.ids[t], &off, &len)) bad = true;
            W->pos += len;
        }
        W->tok = s;
        pos = W->pos;
        if (bad || pos <= b0 || pos >= b1) {               // (the start lies inside the item: nothing is read outside the text)
            simt::atomic_or((unsigned*)&C.counters[0], (unsigned)kErrChunkSum);
            pos = b0;
        }
    }
    if (C.chunk_bytes) C.chunk_bytes[o] = pos - a;
    if (C.chunk_units) C.chunk_units[o] = first ? 0 : pos;
}

TKZ_KERNEL(256) void k_chunk_walk(ChunkParams C, TkzDecodeTable D, int write) {
    const int64_t stride = simt::nblocks() * simt::nthreads(), i0 = simt::bid() * simt::nthreads() + simt::tid();
    const bool bad = C.counters[0] != 0;
    const int64_t m = C.max_tokens;
    if (write) {
        const int64_t nch = C.doc_chunk_offs[C.n_docs];
        if (i0 == 0) *C.n_chunks = nch;
        if (bad || *C.grand > C.out_cap || nch > C.chunk_cap) return;
        if (i0 == 0) C.chunk_tokens[nch] = *C.grand;
    }
    for (int64_t d = i0; d <= C.n_docs; d += stride) {
        if (bad) { if (d < C.n_docs) C.doc_cnt[d] = 0; C.out_offs[d] = 0; continue; }
        const int64_t p0 = C.doc_piece[d];
        int64_t tp = C.piece_toffs[p0];
        if (!write) C.out_offs[d] = tp;
        if (d == C.n_docs) break;
        const int64_t p1 = C.doc_piece[d + 1], tend = C.piece_toffs[p1];
        int64_t c = 0;
        if (tend - tp > m && p1 - p0 > kChunkLongItems) {     // (k_chunk_walk_long's: the count as well)
            if (!write) C.long_list[simt::atomic_add64(C.long_count, 1ull)] = d;
            continue;
        }
        if (tend > tp) {
            const int64_t base = write ? C.doc_chunk_offs[d] : 0, a = write ? C.offs[d] : 0;
            int64_t s = tp, p = p0;
            TkzChunkItem W{-1, 0, 0};
            for (;;) {
                if (write) tkz_chunk_emit(C, D, base + c, a, c == 0, s, p, tp, &W);
                ++c;
                if (tend - s <= m) break;
                s = tkz_chunk_end(C.piece_toffs, p1, s, m, &p, &tp);
            }
        }
        if (!write) C.doc_cnt[d] = c;
    }
}

TKZ_KERNEL(256) void k_chunk_walk_long(ChunkParams C, TkzDecodeTable D, int write) {
    const int lane = simt::lane();
    const int64_t nwaves = simt::nblocks() * (kThreads / 64), wave0 = simt::bid() * (kThreads / 64) + simt::wave();
    if (C.counters[0] != 0) return;                           // (nothing was listed)
    if (write && (*C.grand > C.out_cap || C.doc_chunk_offs[C.n_docs] > C.chunk_cap)) return;
    const int64_t m = C.max_tokens, nlong = (int64_t)*C.long_count, none = (int64_t)0x7FFFFFFFFFFFFFFFll;
    for (int64_t q = wave0; q < nlong; q += nwaves) {
        const int64_t d = C.long_list[q], p0 = C.doc_piece[d], p1 = C.doc_piece[d + 1], tend = C.piece_toffs[p1];
        const int64_t base = write ? C.doc_chunk_offs[d] : 0, a = write ? C.offs[d] : 0;
        int64_t tp = C.piece_toffs[p0], s = tp, p = p0, c = 0;
        // the window: v is piece_toffs[w + lane] (beyond the document: `none`); w <= p + 1 <= w + 63 wherever a chunk starts.  The three windows behind it are
        // on their way (n1, n2, n3): a step to the next window waits for a load issued three steps ago, not for one it has just issued
        int64_t w = p0 + 1;
        const int64_t* const tl = C.piece_toffs + lane;
        int64_t v = w + lane <= p1 ? tl[w] : none, n1 = w + 64 + lane <= p1 ? tl[w + 64] : none, n2 = w + 128 + lane <= p1 ? tl[w + 128] : none,
                n3 = w + 192 + lane <= p1 ? tl[w + 192] : none;
        TkzChunkItem W{-1, 0, 0};
        for (;;) {
            if (write && lane == 0) tkz_chunk_emit(C, D, base + c, a, c == 0, s, p, tp, &W);
            ++c;
            if (tend - s <= m) break;
            const int64_t lim = s + m;
            int64_t k = p, tk = tp;                           // the last boundary at or below lim
            for (;;) {
                const int n = tkz_popc64(simt::ballot(v <= lim));      // (ascending: the lanes at or below lim are the first n)
                if (n > 0 && w + n - 1 > k) { k = w + n - 1; tk = tkz_shfl64(v, n - 1); }
                if (n < 64) break;
                w += 64; v = n1; n1 = n2; n2 = n3; n3 = w + 192 + lane <= p1 ? tl[w + 192] : none;
            }
            if (k > p) { s = tk; p = k; tp = tk; } else s = lim;
        }
        if (!write && lane == 0) C.doc_cnt[d] = c;
    }
}

TKZ_KERNEL(256) void k_chunk_unitcount(ChunkParams C) {
    const int lane = simt::lane();
    const int64_t sub = simt::bid() * (kThreads / 64) + simt::wave();
    if (sub * kSub >= C.total) return;
    uint32_t begun, four;
    tkz_span_units16(C.bytes, C.total, sub * kSub + lane * 16, C.total, &begun, &four);
    int c = tkz_chunk_popc2(begun, four);
    for (int m = 1; m < kChunkUnitSpan / 16; m <<= 1) c += simt::shfl_xor(c, m);
    const int64_t span = sub * (kSub / kChunkUnitSpan) + lane / (kChunkUnitSpan / 16);
    if ((lane & (kChunkUnitSpan / 16 - 1)) == 0 && span < C.nspan) C.cnt_unit[span] = c;
}
// The UTF-16 units begun in [0, x) of the batch (0 <= x < total), by a GROUP of 8 lanes (l8: the lane in its group; every lane of the wavefront calls, every lane
// of a group gets its group's sum): the base of x's span of kChunkUnitSpan bytes and the span's bytes in front of x.  x == 0 reads nothing.
TKZ_DEV int64_t tkz_chunk_units_before(const ChunkParams& C, int64_t x, int l8) {
    int64_t span = x / kChunkUnitSpan;
    if (span >= C.nspan) span = C.nspan - 1;
    const int64_t p0 = span * kChunkUnitSpan + l8 * 16;
    int c = 0;
    if (p0 < x) {
        uint32_t begun, four;
        tkz_span_units16(C.bytes, C.total, p0, x, &begun, &four);
        c = tkz_chunk_popc2(begun, four);
    }
    for (int m = 1; m < kChunkUnitSpan / 16; m <<= 1) c += simt::shfl_xor(c, m);
    return x > 0 ? C.base_unit[span] + c : 0;
}
TKZ_KERNEL(256) void k_chunk_units(ChunkParams C) {
    const int lane = simt::lane(), sl = lane & 15, g0 = lane & 48;
    const int64_t nwaves = simt::nblocks() * (kThreads / 64), wave0 = simt::bid() * (kThreads / 64) + simt::wave();
    const int64_t nch = C.doc_chunk_offs[C.n_docs];
    if (C.counters[0] != 0 || *C.grand > C.out_cap || nch > C.chunk_cap) return;
    for (int64_t c0 = wave0 * 64; c0 < nch; c0 += nwaves * 64) {
        const int64_t c1 = c0 + 64 < nch ? c0 + 64 : nch, c = c0 + lane;
        // the documents of the tile's first and last chunk (wave-uniform), then every lane's own among them
        const int64_t d0 = tkz_last_le(C.doc_chunk_offs, 0, C.n_docs - 1, c0), d1 = tkz_last_le(C.doc_chunk_offs, d0, C.n_docs - 1, c1 - 1);
        int64_t pos = 0, a = 0, units = 0;
        bool work = false;
        if (c < c1) {
            const int64_t d = d0 == d1 ? d0 : tkz_last_le(C.doc_chunk_offs, d0, d1, c);
            if (C.doc_chunk_offs[d] != c) { work = true; pos = C.chunk_units[c]; a = C.offs[d]; }      // (a document's first chunk starts at unit 0: written already)
        }
        if (work && (pos <= a || pos >= C.total)) { pos = a; simt::atomic_or((unsigned*)&C.counters[0], (unsigned)kErrChunkSum); }
        if (!work) pos = a = 0;
        // a group of 16 lanes takes the chunks of its own lanes one after the other, the four groups side by side (the control flow stays wave-uniform: a group
        // with nothing to do counts in front of byte 0, which reads nothing): its lower 8 lanes count in front of the chunk's start, its upper 8 in front of the
        // document's start, at the same time
        for (int r = 0; r < 16; ++r) {
            const int64_t rpos = tkz_shfl64(pos, g0 + r), ra = tkz_shfl64(a, g0 + r);
            if (simt::ballot(rpos != 0) == 0) continue;
            const int64_t mine = tkz_chunk_units_before(C, sl < 8 ? rpos : ra, sl & 7), other = tkz_shfl64(mine, lane ^ 8);
            if (sl == r) units = sl < 8 ? mine - other : other - mine;
        }
        if (work) C.chunk_units[c] = units;
    }
}

// -------------------------------------------------------------------------------------------------
// Token spans (tkz_encode_batch_spans_device): where every token's text starts, behind the piece-granular launch sequence -- which leaves the ids in the
// caller's buffer and the byte and token offset of every piece and the first piece of every document in the workspace.
//   k_tokspan_mark   one lane per piece.  A piece of one token (nearly all, and every taken special-token literal) starts where the piece starts: that bit is in
//                    startbits.  A piece of several tokens walks its ids through the decode table and sets a bit at every INTERIOR token start in `intbits`
//                    (zeroed by the host); key lengths that do not add up to the piece are kErrSpanSum.  The token-start bitmap is startbits | intbits.
//                    The same launch writes the document offsets, out_offs[d] = piece_toffs[doc_piece[d]], and refuses a document of 2^31 bytes or more.
//   k_tokspan_count  one wavefront per sub-tile, a lane per 16 bytes: the token starts and the UTF-16 units begun (one per non-continuation byte, one more per
//                    byte >= 0xF0: k_trim_gather's rule) in the sub-tile.  (k_scan_*: their exclusive scans.)
//   k_tokspan_write  the same walk again: the ordinal of a token-start bit IS the token's index (tokens are ordered by byte), its document starts at the last
//                    document mark at or before it -- in its own lane's 16 bits, in an earlier lane (a maximum scan over the lanes), or in front of the sub-tile
//                    (the 64 bitmap words before it, else one binary search over the offsets per wavefront; for the units the recount of that sub-tile's bytes in front of the
//                    document start).
// An attempt whose counter block holds an error bit, or whose ids did not fit the caller's buffer, leaves the span arrays alone: nothing is promised then.
// -------------------------------------------------------------------------------------------------
// the token-start (or, with intbits null, document-start) bits of the 16 bytes at p0, those at or beyond `total` cleared
TKZ_DEV uint32_t tkz_span_bits16(const uint64_t* bits, const uint64_t* intbits, int64_t total, int64_t p0) {
    const int64_t lim = total - p0;
    if (lim <= 0) return 0u;
    uint64_t w = bits[p0 >> 6];
    if (intbits) w |= intbits[p0 >> 6];
    uint32_t m = (uint32_t)(w >> (p0 & 63)) & 0xFFFFu;
    if (lim < 16) m &= (1u << (int)lim) - 1u;
    return m;
}
// of the 16 bytes at p0 (16-byte aligned; nothing is read at or beyond `total`): bit k of *begun set <=> byte k is no continuation byte, bit k of *four <=> it is
// >= 0xF0 -- the bytes below `end` only
TKZ_DEV void tkz_span_units16(const uint8_t* bytes, int64_t total, int64_t p0, int64_t end, uint32_t* begun, uint32_t* four) {
    uint32_t q[4] = {0u, 0u, 0u, 0u};
    if (p0 + 16 <= total) { const uint4 v = *reinterpret_cast<const uint4*>(bytes + p0); q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w; }
    else for (int k = 0; p0 + k < total; ++k) q[k >> 2] |= (uint32_t)bytes[p0 + k] << (8 * (k & 3));
    uint32_t b = 0, f = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t x = (q[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        b |= ((x & 0xC0u) != 0x80u ? 1u : 0u) << k;
        f |= (x >= 0xF0u ? 1u : 0u) << k;
    }
    const int64_t lim = (end < total ? end : total) - p0;
    const uint32_t keep = lim <= 0 ? 0u : (lim >= 16 ? 0xFFFFu : (1u << (int)lim) - 1u);
    *begun = b & keep; *four = f & keep;
}
TKZ_DEV int tkz_span_units_below(uint32_t begun, uint32_t four, int k) { const uint32_t low = (1u << k) - 1u; return tkz_popc32(begun & low) + tkz_popc32(four & low); }

TKZ_KERNEL(256) void k_tokspan_mark(SpanParams S, TkzDecodeTable D) {
    const int64_t stride = simt::nblocks() * simt::nthreads(), i0 = simt::bid() * simt::nthreads() + simt::tid();
    for (int64_t d = i0; d <= S.n_docs; d += stride) {
        S.out_offs[d] = S.piece_toffs[S.doc_piece[d]];
        if (d < S.n_docs && S.offs[d + 1] - S.offs[d] > (int64_t)0x7FFFFFFF) simt::atomic_or((unsigned*)&S.counters[0], (unsigned)kErrSpanDoc);
    }
    const int64_t g = *S.grand;
    if (S.counters[0] != 0 || g > S.out_cap) return;
    for (int64_t i = i0; i < S.n_pieces; i += stride) {
        const int64_t t0 = S.piece_toffs[i], t1 = S.piece_toffs[i + 1];
        if (t1 - t0 == 1) continue;
        const int64_t b1 = S.piece_boffs[i + 1];
        int64_t pos = S.piece_boffs[i];
        bool bad = t1 <= t0 || t0 < 0 || t1 > g;
        // (four tokens a round: their ids, then their key lengths, are loads that do not wait for one another -- a token at a time was two dependent
        //  round trips a token, and nearly every wavefront has a lane that walks)
        for (int64_t t = t0; !bad && t < t1; t += 4) {
            int32_t id[4];
            uint32_t len[4];
            bool have[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) id[k] = t + k < t1 ? S.ids[t + k] : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { uint32_t off; len[k] = 0; have[k] = t + k < t1 && tkz_dec_find(D, id[k], &off, &len[k]); }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (t + k >= t1 || bad) continue;
                if (!have[k]) { bad = true; continue; }
                pos += len[k];
                if (t + k + 1 == t1) continue;
                if (pos >= b1) bad = true;                  // (an interior start lies inside the piece: nothing is set outside the bitmap)
                else simt::atomic_or64((unsigned long long*)&S.intbits[pos >> 6], 1ull << (pos & 63));
            }
        }
        if (bad || pos != b1) simt::atomic_or((unsigned*)&S.counters[0], (unsigned)kErrSpanSum);
    }
}

TKZ_KERNEL(256) void k_tokspan_count(SpanParams S) {
    const int lane = simt::lane();
    const int64_t sub = simt::bid() * (kThreads / 64) + simt::wave();
    if (sub >= S.nsub) return;
    const int64_t p0 = sub * kSub + lane * 16;
    int tot;
    (void)tkz_wave_scan_sum(tkz_popc32(tkz_span_bits16(S.startbits, S.intbits, S.total, p0)), &tot);
    if (lane == 0) S.cnt_tok[sub] = tot;
    if (!S.tok_units) return;
    uint32_t begun, four;
    tkz_span_units16(S.bytes, S.total, p0, S.total, &begun, &four);
    (void)tkz_wave_scan_sum(tkz_popc32(begun) + tkz_popc32(four), &tot);
    if (lane == 0) S.cnt_unit[sub] = tot;
}

TKZ_KERNEL(256) void k_tokspan_write(SpanParams S) {
    const int lane = simt::lane();
    const int64_t sub = simt::bid() * (kThreads / 64) + simt::wave();
    if (sub >= S.nsub || S.counters[0] != 0 || *S.grand > S.out_cap) return;
    // (as many token starts as there are ids: the marks and the encode kernels agree over the whole batch)
    if (sub == 0 && lane == 0 && S.sums[0] != *S.grand) simt::atomic_or((unsigned*)&S.counters[0], (unsigned)kErrSpanSum);
    const int64_t sub0 = sub * kSub, p0 = sub0 + lane * 16;
    uint32_t m = tkz_span_bits16(S.startbits, S.intbits, S.total, p0);
    const uint32_t dm = tkz_span_bits16(S.docbits, nullptr, S.total, p0);
    int tot;
    int64_t o = S.base_tok[sub] + tkz_wave_scan_sum(tkz_popc32(m), &tot);
    if (tot == 0) return;                                   // (wave-uniform)
    const bool units = S.tok_units != nullptr;
    uint32_t begun = 0, four = 0;
    int upre = 0;                                           // units begun in [sub0, p0)
    if (units) {
        tkz_span_units16(S.bytes, S.total, p0, S.total, &begun, &four);
        int utot;
        upre = tkz_wave_scan_sum(tkz_popc32(begun) + tkz_popc32(four), &utot);
    }
    // the last document start of an EARLIER lane of this sub-tile: (byte in the sub-tile + 1) << 12 | units begun in front of it (< 2,048), ascending with the
    // byte, so the maximum over the lanes in front is the nearest one; 0: none
    int mine = 0;
    if (dm) { const int k = tkz_msb32(dm); mine = ((lane * 16 + k + 1) << 12) | (upre + tkz_span_units_below(begun, four, k)); }
    int run = mine;
    for (int d = 1; d < 64; d <<= 1) { const int y = simt::shfl_up(run, d); if (lane >= d && y > run) run = y; }
    int before = simt::shfl_up(run, 1);
    if (lane == 0) before = 0;
    // ... and the document that is open where the sub-tile begins (wave-uniform; not needed when a document starts at the sub-tile's first byte)
    int64_t in_pos = sub0, in_units = 0;
    if (!(simt::shfl((int)dm, 0) & 1)) {
        // (the last document mark in front of the sub-tile: in the 64 bitmap words before it, a lane a word -- documents of up to 4 KiB --, else by binary search
        //  over the offsets: 24 dependent loads a wavefront on ten million documents were most of this kernel)
        const int64_t w0 = sub0 >> 6, wl = w0 - 1 - lane;
        const uint64_t x = wl >= 0 ? S.docbits[wl] : 0ull;
        const uint64_t found = simt::ballot(x != 0);
        if (found) { const int src = tkz_ctz64(found); in_pos = ((w0 - 1 - src) << 6) + tkz_msb64((uint64_t)tkz_shfl64((int64_t)x, src)); }
        else in_pos = S.offs[tkz_last_le(S.offs, 0, S.n_docs - 1, sub0)];
        if (in_pos < 0) in_pos = 0;
        if (in_pos > sub0) in_pos = sub0;
        if (units) {
            const int64_t isub = in_pos / kSub;
            uint32_t ib, if4;
            tkz_span_units16(S.bytes, S.total, isub * kSub + lane * 16, in_pos, &ib, &if4);
            int itot;
            (void)tkz_wave_scan_sum(tkz_popc32(ib) + tkz_popc32(if4), &itot);
            in_units = S.base_unit[isub] + itot;
        }
    }
    const int64_t ubase = units ? S.base_unit[sub] : 0;
    for (; m; m &= m - 1, ++o) {
        const int k = tkz_ctz32(m);
        const uint32_t dd = dm & ((2u << k) - 1u);          // document starts of this lane at or before bit k
        const int u = units ? upre + tkz_span_units_below(begun, four, k) : 0;
        int64_t boff, uoff;
        if (dd) { const int s = tkz_msb32(dd); boff = k - s; uoff = u - (upre + tkz_span_units_below(begun, four, s)); }
        else if (before) { boff = lane * 16 + k - ((before >> 12) - 1); uoff = u - (before & 0xFFF); }
        else { boff = p0 + k - in_pos; uoff = ubase + u - in_units; }
        if (o < 0 || o >= S.out_cap) continue;
        if (S.tok_bytes) S.tok_bytes[o] = (int32_t)boff;
        if (units) S.tok_units[o] = (int32_t)uoff;
    }
}

// -------------------------------------------------------------------------------------------------
// Overlapping token-budget chunks (tkz_encode_batch_chunks_overlap_device): the chunk section's launch sequence -- count walk, scan, write walk, unit stage -- with
// walks and a unit kernel of their own, so that the kernels of the entries without overlap stay the code they are.  tkz_chunk_end, tkz_chunk_emit,
// tkz_chunk_units_before and k_chunk_unitcount are shared.  The rule (tkz.h): chunk [s, e) ends where the existing rule ends a chunk that starts at s; the next
// one starts at the smallest item boundary in [x, e], x = max(e - overlap, s + 1), at x itself when e lies inside an item, and at e when a chunk begun there
// would end at e again.
//   the next start     e inside an item means that (s, e] holds no boundary: the start is x, in the same item.  Otherwise the boundaries of (s, e] are the
//                      entries ps + 1 .. pe of piece_toffs (ps, pe: the items of s and e), toffs[pe] == e >= x, and the start is the first of them at or above x.
//   adds nothing       a chunk begun at a boundary n < e ends at e again exactly when the boundary behind e lies beyond n + max (e - n <= overlap < max, so e
//                      is in reach): ONE load, toffs[pe + 1], instead of a trial tkz_chunk_end.  A start inside an item never ends at e again (its end is
//                      n + max > e or a boundary behind e), and neither does one whose rest fits the budget (it ends at the document's end, behind e).
//   k_chunkov_walk       one lane per document.  A document of at most max tokens stays two loads.  The start is a binary search over the chunk's own items
//                        ps + 1 .. pe: log2 of the items of a chunk, at most log2(max), loads a chunk beside the galloping search for the end.
//   k_chunkov_walk_long  one wavefront per listed document, the window of k_chunk_walk_long.  The window is NOT stepped back for a start behind it: the end
//                        before (item kf) is at or below the new start + max, so the search for the next end begins there, and w <= kf + 1 <= w + 63 holds
//                        wherever a chunk starts -- the window only moves forward.  The start is searched BACK from the end item: the lanes load the 64
//                        entries that end at pe (they have just passed through the window: cache hits), a ballot of toffs >= x and a population count give
//                        the first, and only an overlap of more than 64 items takes another step back.  A chunk costs one such load of 64 entries per 64
//                        items of overlap and two wave-uniform loads (the start's own entry, the boundary behind e) more than k_chunk_walk_long's.
//   positions            TWO cursors a walk (TkzChunkItem), one for starts and one for ends: inside an oversize item the queries come in the order s, e,
//                        e - overlap < e, each of the two sequences ascends, and neither walks an item's ids from its beginning a second time.  An end at
//                        the document's end is the document's length and reads nothing.
//   k_chunkov_units      k_chunk_units' scheme, once for the starts and once for the ends.  An end may be `total` itself (the last document's last chunk):
//                        tkz_chunk_units_before clamps that position's span to the last one and counts up to `total`, so nothing is read beyond the text.
// Errors as the chunk section: with an error bit the counts are 0; with one, with ids that did not fit or with more chunks than chunk_cap the table is left alone.
// -------------------------------------------------------------------------------------------------
TKZ_DEV int64_t tkz_chunkov_x(int64_t s, int64_t e, int64_t ov) { const int64_t x = e - ov; return x > s + 1 ? x : s + 1; }
TKZ_DEV bool tkz_chunkov_adds_nothing(const int64_t* toffs, int64_t pe, int64_t n, int64_t e, int64_t m) { return n < e && toffs[pe + 1] > n + m; }
// the end of chunk o of the table: token e, in item p (whose first token is tp), of the document [a, aend) of the batch; last: the document's last chunk
TKZ_DEV void tkz_chunkov_emit_end(const ChunkOvParams& V, const TkzDecodeTable& D, int64_t o, int64_t a, int64_t aend, bool last, int64_t e, int64_t p, int64_t tp,
                                  TkzChunkItem* W) {
    const ChunkParams& C = V.C;
    if (o < 0 || o >= C.chunk_cap) return;
    V.chunk_ends[o] = e;
    if (!V.chunk_end_bytes && !V.chunk_end_units) return;
    int64_t pos = aend;
    if (!last && e == tp) pos = C.piece_boffs[p];
    else if (!last) {
        const int64_t b0 = C.piece_boffs[p], b1 = C.piece_boffs[p + 1];
        if (W->item != p) { W->item = p; W->tok = tp; W->pos = b0; }
        bool bad = false;
        for (int64_t t = W->tok; t < e; ++t) {
            uint32_t off, len = 0;
            if (!tkz_dec_find(D, C.ids[t], &off, &len)) bad = true;
            W->pos += len;
        }
        W->tok = e;
        pos = W->pos;
        if (bad || pos <= b0 || pos >= b1) {               // (the end lies inside the item: nothing is read outside the text)
            simt::atomic_or((unsigned*)&C.counters[0], (unsigned)kErrChunkSum);
            pos = b1;
        }
    }
    if (V.chunk_end_bytes) V.chunk_end_bytes[o] = pos - a;
    if (V.chunk_end_units) V.chunk_end_units[o] = pos;
}

TKZ_KERNEL(256) void k_chunkov_walk(ChunkOvParams V, TkzDecodeTable D, int write) {
    const ChunkParams& C = V.C;
    const int64_t stride = simt::nblocks() * simt::nthreads(), i0 = simt::bid() * simt::nthreads() + simt::tid();
    const bool bad = C.counters[0] != 0;
    const int64_t m = C.max_tokens, ov = V.overlap;
    const int64_t* const toffs = C.piece_toffs;
    if (write) {
        const int64_t nch = C.doc_chunk_offs[C.n_docs];
        if (i0 == 0) *C.n_chunks = nch;
        if (bad || *C.grand > C.out_cap || nch > C.chunk_cap) return;
    }
    for (int64_t d = i0; d <= C.n_docs; d += stride) {
        if (bad) { if (d < C.n_docs) C.doc_cnt[d] = 0; C.out_offs[d] = 0; continue; }
        const int64_t p0 = C.doc_piece[d];
        int64_t tp = toffs[p0];
        if (!write) C.out_offs[d] = tp;
        if (d == C.n_docs) break;
        const int64_t p1 = C.doc_piece[d + 1], tend = toffs[p1];
        int64_t c = 0;
        if (tend - tp > m && p1 - p0 > kChunkLongItems) {     // (k_chunkov_walk_long's: the count as well)
            if (!write) C.long_list[simt::atomic_add64(C.long_count, 1ull)] = d;
            continue;
        }
        if (tend > tp) {
            const int64_t base = write ? C.doc_chunk_offs[d] : 0, a = write ? C.offs[d] : 0, aend = write ? C.offs[d + 1] : 0;
            int64_t s = tp, p = p0;
            TkzChunkItem Ws{-1, 0, 0}, We{-1, 0, 0};
            for (;;) {
                const bool last = tend - s <= m;
                int64_t pe = p, tpe = tp, e = tend;
                if (!last) e = tkz_chunk_end(toffs, p1, s, m, &pe, &tpe);
                if (write) {
                    tkz_chunk_emit(C, D, base + c, a, c == 0, s, p, tp, &Ws);
                    tkz_chunkov_emit_end(V, D, base + c, a, aend, last, e, pe, tpe, &We);
                }
                ++c;
                if (last) break;
                const int64_t x = tkz_chunkov_x(s, e, ov);
                if (pe == p) { s = x; continue; }             // (e inside item p: so is the next start)
                int64_t lo = p + 1, hi = pe, n = e;           // the first of toffs[p + 1 .. pe] at or above x: n == toffs[hi] >= x throughout
                while (lo < hi) {
                    const int64_t mid = lo + (hi - lo) / 2, v = toffs[mid];
                    if (v >= x) { hi = mid; n = v; } else lo = mid + 1;
                }
                if (tkz_chunkov_adds_nothing(toffs, pe, n, e, m)) { hi = pe; n = e; }
                s = n; p = hi; tp = n;
            }
        }
        if (!write) C.doc_cnt[d] = c;
    }
}

TKZ_KERNEL(256) void k_chunkov_walk_long(ChunkOvParams V, TkzDecodeTable D, int write) {
    const ChunkParams& C = V.C;
    const int lane = simt::lane();
    const int64_t nwaves = simt::nblocks() * (kThreads / 64), wave0 = simt::bid() * (kThreads / 64) + simt::wave();
    if (C.counters[0] != 0) return;                           // (nothing was listed)
    if (write && (*C.grand > C.out_cap || C.doc_chunk_offs[C.n_docs] > C.chunk_cap)) return;
    const int64_t m = C.max_tokens, ov = V.overlap, nlong = (int64_t)*C.long_count, none = (int64_t)0x7FFFFFFFFFFFFFFFll;
    const int64_t* const toffs = C.piece_toffs;
    for (int64_t q = wave0; q < nlong; q += nwaves) {
        const int64_t d = C.long_list[q], p0 = C.doc_piece[d], p1 = C.doc_piece[d + 1], tend = toffs[p1];
        const int64_t base = write ? C.doc_chunk_offs[d] : 0, a = write ? C.offs[d] : 0, aend = write ? C.offs[d + 1] : 0;
        int64_t tp = toffs[p0], s = tp, p = p0, c = 0;
        // kf: the last item known to begin at or below s + max -- the item of the end before, or the start's own.  The window as in k_chunk_walk_long, with
        // w <= kf + 1 <= w + 63 wherever a chunk starts; it only moves forward
        int64_t kf = p0, tkf = tp;
        int64_t w = p0 + 1;
        const int64_t* const tl = toffs + lane;
        int64_t v = w + lane <= p1 ? tl[w] : none, n1 = w + 64 + lane <= p1 ? tl[w + 64] : none, n2 = w + 128 + lane <= p1 ? tl[w + 128] : none,
                n3 = w + 192 + lane <= p1 ? tl[w + 192] : none;
        TkzChunkItem Ws{-1, 0, 0}, We{-1, 0, 0};
        for (;;) {
            const bool last = tend - s <= m;
            int64_t pe = p, tpe = tp, e = tend;
            if (!last) {
                const int64_t lim = s + m;
                int64_t k = kf, tk = tkf;                     // the last boundary at or below lim
                for (;;) {
                    const int n = tkz_popc64(simt::ballot(v <= lim));      // (ascending: the lanes at or below lim are the first n)
                    if (n > 0 && w + n - 1 > k) { k = w + n - 1; tk = tkz_shfl64(v, n - 1); }
                    if (n < 64) break;
                    w += 64; v = n1; n1 = n2; n2 = n3; n3 = w + 192 + lane <= p1 ? tl[w + 192] : none;
                }
                if (k > p) { e = tk; pe = k; tpe = tk; } else e = lim;
            }
            if (write && lane == 0) {
                tkz_chunk_emit(C, D, base + c, a, c == 0, s, p, tp, &Ws);
                tkz_chunkov_emit_end(V, D, base + c, a, aend, last, e, pe, tpe, &We);
            }
            ++c;
            if (last) break;
            const int64_t x = tkz_chunkov_x(s, e, ov);
            if (pe == p) { s = x; continue; }                 // (e inside item p: so is the next start, and kf == p stays)
            // back from the end item: the entries hi - 63 .. hi, those at or below item p count as below x; the lanes at or above x are the last `back`
            int64_t hi = pe, pn = pe;
            for (;;) {
                const int64_t i = hi - 63 + lane;
                const int64_t u = i > p ? toffs[i] : (int64_t)-1;
                const int back = tkz_popc64(simt::ballot(u >= x));
                pn = hi - back + 1;
                if (back < 64 || hi - 64 <= p) break;
                hi -= 64;
            }
            int64_t n = pn == pe ? e : toffs[pn];
            if (tkz_chunkov_adds_nothing(toffs, pe, n, e, m)) { pn = pe; n = e; }
            s = n; p = pn; tp = n; kf = pe; tkf = e;
        }
        if (!write && lane == 0) C.doc_cnt[d] = c;
    }
}

// The units of 64 positions: every lane's pos and the start a of its document as batch bytes (a lane with nothing to do: both 0, which reads nothing) -> the
// units begun in [a, pos).  k_chunk_units' scheme: a group of 16 lanes takes the positions of its own lanes one after the other, its lower 8 lanes count in front
// of the position, its upper 8 in front of the document's start.  Every lane of the wavefront calls.
TKZ_DEV int64_t tkz_chunkov_units64(const ChunkParams& C, int64_t pos, int64_t a, int lane) {
    const int sl = lane & 15, g0 = lane & 48;
    int64_t units = 0;
    for (int r = 0; r < 16; ++r) {
        const int64_t rpos = tkz_shfl64(pos, g0 + r), ra = tkz_shfl64(a, g0 + r);
        if (simt::ballot(rpos != 0) == 0) continue;
        const int64_t mine = tkz_chunk_units_before(C, sl < 8 ? rpos : ra, sl & 7), other = tkz_shfl64(mine, lane ^ 8);
        if (sl == r) units = sl < 8 ? mine - other : other - mine;
    }
    return units;
}
TKZ_KERNEL(256) void k_chunkov_units(ChunkOvParams V) {
    const ChunkParams& C = V.C;
    const int lane = simt::lane();
    const int64_t nwaves = simt::nblocks() * (kThreads / 64), wave0 = simt::bid() * (kThreads / 64) + simt::wave();
    const int64_t nch = C.doc_chunk_offs[C.n_docs];
    if (C.counters[0] != 0 || *C.grand > C.out_cap || nch > C.chunk_cap) return;
    for (int64_t c0 = wave0 * 64; c0 < nch; c0 += nwaves * 64) {
        const int64_t c1 = c0 + 64 < nch ? c0 + 64 : nch, c = c0 + lane;
        // the documents of the tile's first and last chunk (wave-uniform), then every lane's own among them
        const int64_t d0 = tkz_last_le(C.doc_chunk_offs, 0, C.n_docs - 1, c0), d1 = tkz_last_le(C.doc_chunk_offs, d0, C.n_docs - 1, c1 - 1);
        int64_t a = 0, spos = 0, epos = 0;
        bool first = true;
        if (c < c1) {
            const int64_t d = d0 == d1 ? d0 : tkz_last_le(C.doc_chunk_offs, d0, d1, c);
            first = C.doc_chunk_offs[d] == c;
            a = C.offs[d];
        }
        if (C.chunk_units) {                                  // (a document's first chunk starts at unit 0: written already)
            const bool work = c < c1 && !first;
            if (work) spos = C.chunk_units[c];
            if (work && (spos <= a || spos >= C.total)) { spos = a; simt::atomic_or((unsigned*)&C.counters[0], (unsigned)kErrChunkSum); }
            const int64_t units = tkz_chunkov_units64(C, spos, work ? a : 0, lane);
            if (work) C.chunk_units[c] = units;
        }
        if (V.chunk_end_units) {                              // (every chunk has an end behind its document's start; the last one's may be `total`)
            const bool work = c < c1;
            if (work) epos = V.chunk_end_units[c];
            if (work && (epos <= a || epos > C.total)) { epos = a; simt::atomic_or((unsigned*)&C.counters[0], (unsigned)kErrChunkSum); }
            const int64_t units = tkz_chunkov_units64(C, epos, work ? a : 0, lane);
            if (work) V.chunk_end_units[c] = units;
        }
    }
}

// -------------------------------------------------------------------------------------------------
// k_small: the WHOLE launch sequence for a small batch in ONE kernel, one workgroup (ITokenizer.Encode of a prompt, TikTokenizer.cs:178-207;
// the shape of BASELINE.json configs[0]).  The batch path above is ~25 launches and as many dependent kernel boundaries: ~160 us for a
// 64-byte prompt, whatever the kernels do.  Here the phases are the same device functions (tkz_probe_subtile, tkz_merge_short_group,
// tkz_merge_long_chunks, tkz_place_subtiles), run one after the other by the four wavefronts of one workgroup with a workgroup
// barrier between them; the text and the offsets are read straight from page-locked host memory and the ids, the document offsets and
// the status go straight back into it: one launch, one stream synchronisation, no copy commands.
//   limits (checked by the host): total <= kSmallMaxBytes (128 sub-tiles), n_docs <= kSmallMaxDocs; o200k, which has no row evaluator and is
//   split by the sequential matcher -- the definition -- one lane per document over text staged in LDS: total <= kSmallMaxBytesO200k and
//   every document <= kSmallMaxDoc bytes
//   a giant piece, a missed piece of more than kLanePiece bytes (k_merge_coop's), a miss list or record buffer that is too small: status != 0, and the
//   host takes the batch path (which has the retries)
// SPECIAL (tkz_encode_special_utf8 / _utf16: Encode(text, allowedSpecial) on one string): the literal search of the special entries in the same launch --
//   tkz_lit_scan_block, tkz_lit_resolve_word between the document marks and the pre-tokenizer, which then splits between SEGMENT marks; tkz_lit_fix_word behind
//   it; tkz_probe_subtile<true, true>.  Each of these phases reads from memory what the one before wrote there (atomic ORs and plain stores of the same
//   workgroup): a workgroup barrier between them orders that, as it does for the document marks.  The literal phase lives in the one LDS block: the table as
//   k_lit_scan stages it (2,112 B of meta + 32 KB of blob at their limits) and a text stage per wavefront of kSmallLitBlock + kLitMaxLen bytes -- 2 KiB blocks,
//   not k_lit_scan's 4 KiB: sixteen of those beside the table are 102 KB, over the 83.5 KB the pre-tokenizer phase needs anyway; sixteen of these are 69.7 KB.
//   The table stays in LDS because a lane whose byte is in the set of first bytes walks all of it.  SPECIAL == false compiles to the code it always was.
// TRIM (tkz_encode_trim_utf8 / _utf16: EncodeTrimSuffix / EncodeTrimPrefix of ONE string; either SPECIAL): the batch trim path's launch sequence in the same
//   launch.  The marks the encode phases see are the PIECE starts, behind tkz_lit_fix_word (the host binds EncodeParams::docbits to the piece-start bitmap, as
//   enqueue_attempt does for CallKind::Pieces): doc_tok receives a token position per piece, a taken literal is one item of one token, and phase 3 counts its
//   "documents" from that bitmap.  Behind the place phase comes the cut, k_trim_cut's rule: the tokens in front of the piece boundary at byte pos are
//   tile_base[sub] + doc_tok[ordinal(pos)] -- strictly ascending, every item has a token --; the bitmap words are dealt out to the threads, each walks its set
//   bits, and a workgroup-wide maximum (suffix: the last boundary with at most `max` in front of it, byte 0 when none) or minimum (prefix: the first with at
//   least count - max, `total` when none) follows through a few words of the LDS block.  Then cut_units as k_trim_gather counts them, over the quads of
//   [0, cut).  Nothing is gathered: the untrimmed ids are in the page-locked block and the host copies [first, first + kept).  TRIM == false compiles to the
//   code it always was.
// -------------------------------------------------------------------------------------------------
constexpr int kSmallLitBlock = 2048;       // bytes of text per wavefront and round of the literal scan (32 bitmap words)
constexpr int kSmallLitTextQuads = (kSmallLitBlock + kLitMaxLen) / 16, kSmallLitTableQuads = kLitMetaWords / 4 + kLitBlobQuads;
constexpr int kSmallWaves = 16;            // the workgroup is 256 threads for up to 4 sub-tiles, 1024 beyond
constexpr int kSmallLdsQuads = kSmallWaves * kPretokBlkQuads + 16;       // 83.5 KB: the largest phase (a 4 KiB block of the pre-tokenizer per wavefront)
static_assert(kSmallLdsQuads >= kSmallWaves * kProbeLdsQuads + kProbeMaskRows && kSmallLdsQuads >= 8 * kMsLdsQuads + 32 && kSmallLdsQuads >= kLongLdsQuads &&
              kSmallLdsQuads >= kSmallWaves * kPlaceLdsQuads && kSmallLdsQuads * 16 >= kSmallMaxBytesO200k + 64 && kSmallMaxBytes <= 8 * kGroup * kSub,
              "every phase fits the one LDS block; the o200k text too; at most 8 groups of k_merge_short");
static_assert(kLitMetaWords % 4 == 0 && kSmallLdsQuads >= kSmallLitTableQuads + kSmallWaves * kSmallLitTextQuads &&
              kSmallLdsQuads >= kSmallWaves * kProbeLdsQuads + kProbeMaskRows + kSmallWaves * (kSub / 128),
              "the literal phase fits the one LDS block as well, and the probe phase with the words of the literals' starts");
template <bool SPECIAL, bool TRIM = false>
TKZ_KERNEL(1024) void k_small(TkzTables T, EncodeParams P, SmallArgs A) {
    static_assert(kSmallLdsQuads * 16 <= kSmallLdsBytesNeeded, "tkz_kernels.h: what the host checks against the device's LDS per workgroup");
    static_assert(kSmallLdsBytesNeeded == 86 * 1024, "the special form takes no more LDS than the plain one always did");
    TKZ_SHARED uint4 s_raw[kSmallLdsQuads];
    TKZ_SHARED int s_flag;
    const int tid = simt::tid(), lane = simt::lane(), wave = simt::wave();
    const int kThreads = simt::nthreads(), nwaves = kThreads >> 6;          // (shadows the constant: every stride below is the actual workgroup size)
    const int64_t total = P.total, n_docs = P.n_docs, nwords = P.nwords;
    const int nsub = (int)P.nsub;
    uint8_t* const d_bytes = const_cast<uint8_t*>(P.bytes);
    int64_t* const d_offs = const_cast<int64_t*>(P.offs);
    uint8_t* const s_text = reinterpret_cast<uint8_t*>(s_raw);
    int stamp_i = 4;                                              // h_result[4..]: the shader clock at the end of every phase (thread 0)
    auto stamp = [&]() { if (tid == 0 && stamp_i < 20) A.h_result[stamp_i] = (int64_t)simt::clock(); ++stamp_i; };
    stamp();
    // ---- 0. the input from page-locked host memory into HBM (the later phases gather from it) and into LDS (the matcher reads it char by
    // char); everything the phases accumulate into, zeroed ----
    for (int64_t i = tid; 16 * i < total; i += kThreads) {
        uint4 v = tkz_load16(A.h_bytes + 16 * i);                 // (the host buffer is kSmallMaxBytes + 64 long: whole quads can be read)
        if (16 * i + 16 > total) {                               // bytes beyond the text read as 0
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
            for (int j = 0; j < 16; ++j) if (16 * i + j >= total) w[j >> 2] &= ~(0xFFu << (8 * (j & 3)));
            v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        }
        *reinterpret_cast<uint4*>(d_bytes + 16 * i) = v;
        if (!SPECIAL && tkz_pat_is_o200k(T.pattern)) s_raw[i] = v;   // (only the sequential matcher reads the text from LDS; SPECIAL: behind the literal phase)
    }
    for (int64_t d = tid; d <= n_docs; d += kThreads) d_offs[d] = A.h_offs[d];
    for (int64_t w = tid; w < nwords + 1; w += kThreads) A.docbits[w] = 0;
    for (int i = tid; i < A.counter_words; i += kThreads) P.counters[i] = 0;
    for (int t = tid; t < nsub; t += kThreads) P.heavy_flag[t] = 0;
    if (tid == 0) s_flag = 0;
    simt::sync();
    stamp();
    // ---- 1. document marks (k_docmark) ----
    for (int64_t d = tid; d <= n_docs; d += kThreads) {
        const int64_t pos = d_offs[d];
        bool ok = pos >= 0 && pos <= total;
        if (d == 0) ok = ok && pos == 0;
        if (d == n_docs) ok = ok && pos == total;
        else ok = ok && pos <= d_offs[d + 1];
        if (!ok) { simt::atomic_or((unsigned*)&P.counters[0], (unsigned)kErrOffsets); continue; }
        simt::atomic_or64((unsigned long long*)&A.docbits[pos >> 6], 1ull << (pos & 63));
    }
    simt::sync();
    for (int64_t w = tid; w < nwords; w += kThreads) A.startbits[w] = A.docbits[w];
    simt::sync();
    stamp();
    // ---- 1s. the literals taken (k_lit_scan: the blocks dealt out to the wavefronts; k_lit_resolve: the words dealt out to the threads) ----
    const uint64_t* isobits = A.docbits;                          // what the pre-tokenizer splits between: documents, or (SPECIAL) segments
    if constexpr (SPECIAL) {
        uint32_t* s_meta = reinterpret_cast<uint32_t*>(s_raw);
        uint4* s_blob = s_raw + kLitMetaWords / 4;
        tkz_lit_stage_table(A.lit, s_meta, s_blob);
        simt::sync();
        for (int64_t blk = wave; blk * (kSmallLitBlock / 64) < nwords; blk += nwaves) {
            (void)simt::ballot(true);                             // (the block before this one is no longer read)
            tkz_lit_scan_block<kSmallLitBlock>(blk, s_raw + kSmallLitTableQuads + wave * kSmallLitTextQuads, s_meta, s_blob, d_bytes, total, A.docbits, nwords, A.lit.n,
                                               A.allowed, A.candbits, A.segbits, A.specbits, A.endbits, A.repl);
        }
        simt::sync();
        stamp();
        unsigned long long taken = 0;
        for (int64_t w = tid; w < nwords; w += kThreads)
            taken += tkz_lit_resolve_word(w, d_bytes, total, A.docbits, A.candbits, nwords, A.lit, A.segbits, A.specbits, A.endbits, A.repl);
        if (taken) simt::atomic_add64(A.n_taken, taken);
        simt::sync();
        // (the sequential matcher ORs its starts into the segment marks; its text moves into LDS now that the literal table is done with)
        for (int64_t w = tid; w < nwords; w += kThreads) A.startbits[w] = A.segbits[w];
        if (tkz_pat_is_o200k(T.pattern)) for (int64_t i = tid; 16 * i < total; i += kThreads) s_raw[i] = *reinterpret_cast<const uint4*>(d_bytes + 16 * i);
        simt::sync();
        stamp();
        isobits = A.segbits;
    }
    // ---- 2. Regex.Matches.  Pattern 1 / cl100k: the row evaluator (one lane per BYTE of a 64-byte row, rows one after the other, scan state
    // carried: tkz_rows_sequential), the rows dealt out to the four wavefronts -- the sequential matcher took 55 us for a 64-byte prompt
    // (thousands of dependent reads), this takes ~2.  o200k has no row evaluator: the matcher, one lane per document, on the text in LDS ----
    if (SPECIAL && tkz_pat_is_o200k(T.pattern)) {
        // one lane per SEGMENT: the marks of a bitmap word by one thread, a segment's end from the next mark (the bitmap ends in one at `total`)
        for (int64_t w = tid; w < nwords; w += kThreads) {
            for (uint64_t m = isobits[w]; m; m &= m - 1) {
                const int bit = tkz_ctz64(m);
                const int64_t a = (w << 6) + bit;
                if (a >= total) continue;
                int64_t b = total;
                uint64_t nx = bit == 63 ? 0ull : isobits[w] & ~tkz_lowmask(bit + 1);
                for (int64_t v = w; ; nx = isobits[v]) {
                    if (nx) { b = (v << 6) + tkz_ctz64(nx); break; }
                    if (++v >= nwords) break;
                }
                if (b > total) b = total;
                TkzDoc doc; doc.b = s_text + a; doc.n = b - a; doc.bmp = T.bmp_class; doc.by_code_point = T.pattern == TKZ_PAT_O200K;
                int bad = 0;
                for (int64_t p = 0; p < doc.n;) { const TkzChar c = tkz_doc_char(doc, p); bad |= c.bad; p += c.len; }
                if (bad) { simt::atomic_or((unsigned*)&P.counters[0], (unsigned)kErrUtf8); continue; }
                tkz_seq_emit(T.pattern, doc, a, 0, a, b, A.startbits);
            }
        }
    } else if (tkz_pat_is_o200k(T.pattern)) {
        for (int64_t d = tid; d < n_docs; d += kThreads) {
            const int64_t a = d_offs[d], b = d_offs[d + 1];
            if (b <= a || a < 0 || b > total) continue;
            TkzDoc doc; doc.b = s_text + a; doc.n = b - a; doc.bmp = T.bmp_class; doc.by_code_point = T.pattern == TKZ_PAT_O200K;
            int bad = 0;
            for (int64_t p = 0; p < doc.n;) { const TkzChar c = tkz_doc_char(doc, p); bad |= c.bad; p += c.len; }
            if (bad) { simt::atomic_or((unsigned*)&P.counters[0], (unsigned)kErrUtf8); continue; }
            tkz_seq_emit(T.pattern, doc, a, 0, a, b, A.startbits);
        }
    } else {
        simt::sync();                                             // (the text in LDS is not needed on this path: its place take the flag table and the blocks)
        uint16_t* s_aflags = reinterpret_cast<uint16_t*>(s_raw + kSmallWaves * kPretokBlkQuads);
        for (int i = tid; i < 128; i += kThreads) s_aflags[i] = (uint16_t)tkz_ascii_flags((uint32_t)i, T.pattern == TKZ_PAT_CL100K);
        simt::sync();
        for (int64_t blk = wave; blk * kRowsPerWave < nwords; blk += nwaves) {
            if (T.pattern == TKZ_PAT_P1) tkz_pretok_block<TKZ_PAT_P1>(blk, s_raw + wave * kPretokBlkQuads, s_aflags, d_bytes, total, isobits, A.startbits, nwords, T.bmp_class, P.counters);
            else tkz_pretok_block<TKZ_PAT_CL100K>(blk, s_raw + wave * kPretokBlkQuads, s_aflags, d_bytes, total, isobits, A.startbits, nwords, T.bmp_class, P.counters);
        }
    }
    simt::sync();
    stamp();
    if constexpr (SPECIAL) {                                      // (every taken literal ONE piece: k_lit_fix)
        for (int64_t w = tid; w < nwords; w += kThreads) tkz_lit_fix_word(w, A.startbits, A.segbits, A.specbits, A.endbits);
        simt::sync();
        stamp();
    }
    // ---- 3. documents and pieces that start in each sub-tile, their scans (k_doccount2 + k_scan_*): one lane per sub-tile ----
    if (wave == 0) {
        int dcarry = 0, pcarry = 0;
        for (int q0 = 0; q0 < nsub; q0 += 64) {                   // 64 sub-tiles per round, one per lane
            const int q = q0 + lane;
            int dc = 0, pc = 0;
            if (q < nsub) {
                for (int k = 0; k < kSub / 64; ++k) {
                    const int64_t w = (int64_t)q * (kSub / 64) + k;
                    uint64_t md = w < nwords ? A.docbits[w] : 0ull, mp = w < nwords ? A.startbits[w] : 0ull;
                    const int64_t lim = total - (w << 6);                  // (the sentinel bit at `total` is not a start)
                    if (lim <= 0) { md = 0; mp = 0; } else if (lim < 64) { md &= tkz_lowmask((int)lim); mp &= tkz_lowmask((int)lim); }
                    if constexpr (TRIM) md = mp;                           // (a mark, and a doc_tok entry, per PIECE)
                    dc += tkz_popc64(md); pc += tkz_popc64(mp);
                }
            }
            int dtot, ptot;
            const int dpre = dcarry + tkz_wave_scan_sum(dc, &dtot);
            const int ppre = pcarry + tkz_wave_scan_sum((pc + kRecordLine - 1) & ~(kRecordLine - 1), &ptot);
            if (q < nsub) { A.docord_base[q] = dpre; A.pcount[q] = pc; A.pbase[q] = ppre; }
            dcarry += dtot; pcarry += ptot;
        }
        if (lane == 0 && pcarry > P.prank_cap) simt::atomic_or((unsigned*)&P.counters[0], (unsigned)kErrCapacity);
    }
    simt::sync();
    stamp();
    // ---- 4. whole-piece lookups (k_probe) ----
    {
        uint4* s_kmask = s_raw + nwaves * kProbeLdsQuads;
        tkz_probe_kmask_init(s_kmask);
        simt::sync();
        for (int sub = wave; sub < nsub; sub += nwaves) {
            ProbeText tx;
            tkz_probe_request_text(P, sub, &tx);
            ProbeLds LD = tkz_probe_lds(s_raw + wave * kProbeLdsQuads, s_kmask);
            if constexpr (SPECIAL) LD.spec = reinterpret_cast<uint32_t*>(s_kmask + kProbeMaskRows + wave * (kSub / 128));      // (k_probe_special's s_spec: behind the mask table)
            tkz_probe_subtile<true, SPECIAL>(T, P, sub, LD, tx, -1);
            (void)simt::ballot(true);
        }
    }
    simt::sync();
    if (tid == 0) { int f = P.counters[0] != 0; for (int t = 0; t < nsub; ++t) f |= (P.heavy_flag[t] & 2u) != 0; s_flag = f; }
    simt::sync();
    if (s_flag) {                                                 // a giant piece, an error, a buffer that is too small: the batch path's business
        if (tid == 0) { A.h_result[0] = 1; A.h_result[1] = P.counters[0]; }
        return;
    }
    stamp();
    // ---- 5. BytePairEncode of the short misses (k_merge_short: one group of 16 sub-tiles), then of the long ones (k_merge_long: one chunk) ----
    {
        uint16_t* s_brank16 = reinterpret_cast<uint16_t*>(s_raw + 8 * kMsLdsQuads);
        tkz_ms_brank_init(T, s_brank16);
        simt::sync();
        for (int g = wave; g < 8 && g * kGroup < nsub; g += nwaves) tkz_merge_short_group(T, P, g, tkz_ms_lds(s_raw + wave * kMsLdsQuads, s_brank16));
    }
    simt::sync();
    stamp();
    if (wave == 0) {
        const LongLds LD = tkz_long_lds(s_raw);
        tkz_long_brank_init(T, LD.brank);
        if (T.max_rank <= kVarCompactMaxRank) tkz_merge_long_chunks<true>(T, P, 0, 1, LD, kSmallLanePiece);
        else tkz_merge_long_chunks<false>(T, P, 0, 1, LD, kSmallLanePiece);
    }
    simt::sync();
    stamp();
    // ---- 6. scan of the token counts (k_scan_*), ids to their places (k_place), document offsets (k_docoffs) ----
    if (wave == 0) {
        int carry = 0;
        for (int q0 = 0; q0 < nsub; q0 += 64) {
            const int q = q0 + lane;
            int tot;
            const int pre = carry + tkz_wave_scan_sum(q < nsub ? P.tile_count[q] : 0, &tot);
            if (q < nsub) A.tile_base[q] = pre;
            carry += tot;
        }
        if (lane == 0) { A.h_result[2] = carry; A.tile_base[nsub] = carry; }
    }
    simt::sync();
    stamp();
    for (int s0 = wave * kPlacePer; s0 < nsub; s0 += nwaves * kPlacePer)
    {
        if (P.promo) tkz_place_subtiles<64, true, kStageMin>(P, A.tile_base, A.out, A.out_cap, s0, tkz_place_lds<64, kStageMin>(s_raw + wave * kPlaceLdsQuads));
        else tkz_place_subtiles<64, false, kStageMin>(P, A.tile_base, A.out, A.out_cap, s0, tkz_place_lds<64, kStageMin>(s_raw + wave * kPlaceLdsQuads));
    }
    simt::sync();
    stamp();
    {
        const int64_t grand = A.tile_base[nsub];
        const uint64_t* const marks = TRIM ? A.startbits : A.docbits;
        for (int64_t d = tid; d <= n_docs; d += kThreads) {
            const int64_t pos = d_offs[d];
            if (pos >= total) { A.out_offs[d] = grand; continue; }
            const int64_t sub = pos / kSub, wpos = pos >> 6;
            int64_t ord = A.docord_base[sub];
            for (int64_t w = sub * (kSub / 64); w < wpos; ++w) ord += tkz_popc64(marks[w]);
            ord += tkz_popc64(marks[wpos] & tkz_lowmask((int)(pos & 63)));
            A.out_offs[d] = A.tile_base[sub] + P.doc_tok[ord];
        }
    }
    simt::sync();
    stamp();
    [[maybe_unused]] int64_t trim_kept = 0;
    if constexpr (TRIM) {
        // ---- 7. the cut (k_trim_cut's rule over the piece boundaries of the one document), then cut_units (k_trim_gather's second half) ----
        int64_t* const s_cut = reinterpret_cast<int64_t*>(s_raw);          // [0 .. 2 nwaves): the wavefronts' boundaries; [32 .. 32 + nwaves): their unit counts
        const int64_t grand = A.tile_base[nsub], m = A.trim_max, need = grand - m;
        const bool suffix = A.trim_side == 0, whole = grand <= m;
        // (the boundary at `total` has `grand` in front of it: a text kept whole is cut there for suffix and at byte 0 for prefix; a text that is cut starts
        //  from "no boundary qualifies": byte 0 for suffix, `total` -- which qualifies, need <= grand -- for prefix)
        int64_t bpos = suffix == whole ? total : 0, bcnt = suffix == whole ? grand : 0;
        if (!whole) {
            for (int64_t w = tid; w < nwords; w += kThreads) {
                uint64_t mk = A.startbits[w];
                const int64_t lim = total - (w << 6);                      // (the sentinel bit at `total` is not a start)
                if (lim < 64) mk &= tkz_lowmask((int)(lim < 0 ? 0 : lim));
                if (!mk) continue;
                const int64_t sub = w / (kSub / 64), tb = A.tile_base[sub];
                int64_t ord = A.docord_base[sub];
                for (int64_t v = sub * (kSub / 64); v < w; ++v) ord += tkz_popc64(A.startbits[v]);
                for (; mk; mk &= mk - 1, ++ord) {
                    const int64_t pos = (w << 6) + tkz_ctz64(mk), cnt = tb + P.doc_tok[ord];
                    if (suffix) { if (cnt > m) break; if (pos >= bpos) { bpos = pos; bcnt = cnt; } }
                    else if (cnt >= need) { if (pos < bpos) { bpos = pos; bcnt = cnt; } break; }
                }
            }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const int64_t op = tkz_shfl64(bpos, lane ^ d), oc = tkz_shfl64(bcnt, lane ^ d);
            if (suffix ? op > bpos : op < bpos) { bpos = op; bcnt = oc; }
        }
        if (lane == 0) { s_cut[2 * wave] = bpos; s_cut[2 * wave + 1] = bcnt; }
        simt::sync();
        for (int k = 0; k < nwaves; ++k) {
            const int64_t op = s_cut[2 * k], oc = s_cut[2 * k + 1];
            if (suffix ? op > bpos : op < bpos) { bpos = op; bcnt = oc; }
        }
        stamp();
        // a unit per non-continuation byte and one more per byte >= 0xF0, a quad of [0, cut) a thread; the bytes of the last quad at and behind the cut count
        // as continuation bytes
        int units = 0;
        for (int64_t q = tid; 16 * q < bpos; q += kThreads) {
            const uint4 v = *reinterpret_cast<const uint4*>(d_bytes + 16 * q);
            const uint32_t x4[4] = {v.x, v.y, v.z, v.w};
            for (int j = 0; j < 4; ++j) {
                const int64_t r = bpos - 16 * q - 4 * j;                   // bytes of this dword in front of the cut
                if (r <= 0) break;
                uint32_t x = x4[j];
                if (r < 4) x = (x & (0xFFFFFFFFu >> (8 * (4 - (int)r)))) | (0x80808080u << (8 * (int)r));
                units += 4 - tkz_popc32(x & ~(x << 1) & 0x80808080u) + tkz_popc32(x & (x << 1) & (x << 2) & (x << 3) & 0x80808080u);
            }
        }
        int wtot;
        (void)tkz_wave_scan_sum(units, &wtot);
        if (lane == 0) s_cut[32 + wave] = wtot;
        simt::sync();
        if (tid == 0) {
            int64_t cu = 0;
            for (int k = 0; k < nwaves; ++k) cu += s_cut[32 + k];
            trim_kept = suffix ? bcnt : grand - bcnt;
            A.h_result[20] = suffix ? 0 : bcnt; A.h_result[21] = trim_kept; A.h_result[22] = bpos; A.h_result[23] = cu;
        }
        stamp();
    }
    if (tid == 0) {
        const int32_t err = P.counters[0]; A.h_result[1] = err; A.h_result[0] = err ? 1 : 0;
        if constexpr (SPECIAL) {
            A.h_result[3] = (int64_t)*A.n_taken;
            if (P.stats && !err) {                                // TKZ_OPT_PIECE_STATS: k_miss_stats
                unsigned long long ns = 0, nl = 0, np = 0;
                for (int t = 0; t < nsub; ++t) { const uint32_t m = P.mcount[t]; ns += m & 0xFFFFu; nl += m >> 16; np += (unsigned long long)A.pcount[t]; }
                simt::atomic_add64(&P.stats[2], ns); simt::atomic_add64(&P.stats[3], nl); simt::atomic_add64(&P.stats[4], np);
            }
        }
        // {n_docs, n_bytes, n_tokens} of this batch on the device, as k_counts3 leaves them on the batch path (a batch that is handed back
        // gets them from there)
        if (!err) for (int k = 0; k < 2; ++k) if (A.counts3[k]) { A.counts3[k][0] = n_docs; A.counts3[k][1] = total; A.counts3[k][2] = TRIM ? trim_kept : A.tile_base[nsub]; }
    }
}

// -------------------------------------------------------------------------------------------------
// k_dec_small: Decode of ONE id list in ONE kernel, one workgroup (ITokenizer.Decode after a generation, TikTokenizer.cs:586-604; a streaming host calls it
// every few tokens).  The batch entries are two uploads, ~12 launches, two waits and two downloads whatever the size; here the phases are the same device
// functions (tkz_dec_lane, tkz_u8_lane, tkz_u8_stage), run one after the other by the wavefronts of one workgroup with workgroup barriers between them -- no
// atomics, nothing spins on memory.  The ids are read straight from page-locked host memory and the result and its record go straight back into it.
//   1  lengths: the 1024-id tiles dealt out to the wavefronts round-robin (k_dec_len); the tile sums into LDS
//   2  their exclusive scan in LDS (the first wavefront); more than kDecSmallMaxBytes bytes: status 1, the host takes the batch path
//   3  the bytes, staged per tile in LDS and stored coalesced; a tile of more than kDecSmallStage bytes is copied directly (k_dec_write).  A wavefront's first
//      tile keeps its table entries in registers from phase 1.  UTF-8 form: into the page-locked block, done.
//   UTF-16 form (Encoding.UTF8.GetString, the k_u8_* family): phase 3 writes the bytes to the workspace, with the one document's start bitmap -- bit 0 and the
//   sentinel at the total, nothing else -- beside them                                                                        | barrier
//   4  unit counts per 1024-byte tile (k_u8_len), 5 their scan, 6 the units staged in LDS and stored coalesced into the block (k_u8_write)
// LDS: kDecSmallWaves stages of kDecSmallStage bytes (sixteen of k_dec_write's 12 KiB would be 192 KB; 5 KiB holds a tile of English text, ~4.4 bytes an id, and
// phase 6's kU8Stage units) + the sums and bases of up to 128 tiles: 82,960 bytes a workgroup in the compiler's report, inside kSmallLdsBytesNeeded, which the host has checked against the device.
// -------------------------------------------------------------------------------------------------
constexpr int kDecSmallWaves = 16;         // the workgroup is 256 threads for up to 4 id tiles, 1024 beyond
constexpr int kDecSmallStage = 5120;       // bytes of LDS stage per wavefront
constexpr int kDecSmallTiles = kDecSmallMaxBytes / kU8Tile;       // the most tiles either scan sees
static_assert(kDecSmallMaxIds % kDecTile == 0 && kDecSmallMaxIds / kDecTile <= kDecSmallTiles && kDecSmallMaxBytes % kU8Tile == 0, "whole tiles; one scan buffer serves both families");
static_assert(kDecSmallStage % 16 == 0 && kU8Stage * 2 <= kDecSmallStage, "a wavefront's stage holds the units of a byte tile as well");
static_assert(kDecSmallWaves * kDecSmallStage + (2 * kDecSmallTiles + 1) * 4 <= kSmallLdsBytesNeeded, "tkz_kernels.h: what the host checks against the device's LDS per workgroup");
// exclusive scan of n <= kDecSmallTiles tile sums in LDS by the first wavefront, the total in s_base[n]; a workgroup barrier on either side
TKZ_DEV void tkz_dec_small_scan(const int* s_sum, int* s_base, int n) {
    simt::sync();
    if (simt::wave() == 0) {
        int carry = 0;
        for (int q0 = 0; q0 < n; q0 += 64) {
            const int q = q0 + simt::lane();
            int tot;
            const int pre = carry + tkz_wave_scan_sum(q < n ? s_sum[q] : 0, &tot);
            if (q < n) s_base[q] = pre;
            carry += tot;
        }
        if (simt::lane() == 0) s_base[n] = carry;
    }
    simt::sync();
}
template <bool UTF16>
TKZ_KERNEL(1024) void k_dec_small(TkzDecodeTable D, DecSmallArgs A) {
    TKZ_SHARED uint4 s_stage[kDecSmallWaves * kDecSmallStage / 16];
    TKZ_SHARED int s_sum[kDecSmallTiles], s_base[kDecSmallTiles + 1];
    const int tid = simt::tid(), lane = simt::lane(), wave = simt::wave();
    const int nthreads = simt::nthreads(), nwaves = nthreads >> 6;
    uint8_t* const st = reinterpret_cast<uint8_t*>(s_stage) + wave * kDecSmallStage;       // (private to the wavefront: its LDS accesses are ordered, no barrier)
    int stamp_i = 4;                                              // h_result[4..]: the shader clock at the end of every phase (thread 0), as k_small leaves them
    auto stamp = [&]() { if (tid == 0 && stamp_i < 20) A.h_result[stamp_i] = (int64_t)simt::clock(); ++stamp_i; };
    stamp();
    const int64_t n_ids = A.n_ids;
    const int ntiles = (int)((n_ids + kDecTile - 1) / kDecTile);
    // ---- 1. byte length of every id (k_dec_len) ----
    TkzDecLane L0 = {};
    int sum0 = 0;
    for (int t = wave; t < ntiles; t += nwaves) {
        TkzDecLane L;
        const int sum = tkz_dec_lane(D, A.h_ids, n_ids, t, &L);
        // (an entry longer than the block -- only a registered literal can be -- hands the list back before any sum of such lengths is formed: the sums below stay
        //  far inside an int, and phase 3 only ever sees tiles whose bytes end inside the block)
        bool big = false;
#pragma unroll
        for (int k = 0; k < kDecLane; ++k) big = big || L.len[k] > (uint32_t)kDecSmallMaxBytes;
        const bool anybig = simt::ballot(big) != 0;
        int tot;
        (void)tkz_wave_scan_sum(anybig ? 0 : sum, &tot);
        if (anybig || tot > kDecSmallMaxBytes) tot = kDecSmallMaxBytes + 1;
        if (lane == 0) s_sum[t] = tot;
        if (t == wave) { L0 = L; sum0 = sum; }
    }
    stamp();
    // ---- 2. scan of the tile sums ----
    tkz_dec_small_scan(s_sum, s_base, ntiles);
    const int nbytes = s_base[ntiles];
    if (nbytes > kDecSmallMaxBytes) {                             // (workgroup-uniform) more than the block holds: the batch path's business
        if (tid == 0) { A.h_result[1] = nbytes; A.h_result[0] = 1; }
        return;
    }
    stamp();
    // ---- 3. the bytes (k_dec_write) ----
    uint8_t* const out8 = UTF16 ? A.d_bytes : static_cast<uint8_t*>(A.h_out);
    for (int t = wave; t < ntiles; t += nwaves) {
        TkzDecLane L;
        int sum;
        if (t == wave) { L = L0; sum = sum0; } else sum = tkz_dec_lane(D, A.h_ids, n_ids, t, &L);
        int tot;
        int pos = tkz_wave_scan_sum(sum, &tot);
        uint8_t* const dst = out8 + s_base[t];                    // (s_base[t] + tot <= nbytes <= kDecSmallMaxBytes)
        if (tot <= kDecSmallStage) {
#pragma unroll 1
            for (int k = 0; k < kDecLane; ++k) { const uint8_t* src = D.blob + L.off[k]; for (uint32_t j = 0; j < L.len[k]; ++j) st[pos + (int)j] = src[j]; pos += (int)L.len[k]; }
            (void)simt::ballot(true);
            for (int i = lane; i < tot; i += 64) dst[i] = st[i];
            (void)simt::ballot(true);                             // (the wavefront's next tile stages behind these reads)
        } else {
#pragma unroll 1
            for (int k = 0; k < kDecLane; ++k) { const uint8_t* src = D.blob + L.off[k]; for (uint32_t j = 0; j < L.len[k]; ++j) dst[pos + (int)j] = src[j]; pos += (int)L.len[k]; }
        }
    }
    if constexpr (UTF16) {
        const int64_t nwords = nbytes / 64 + 1;
        for (int64_t w = tid; w < nwords; w += nthreads)
            A.d_docbits[w] = (w == 0 ? 1ull : 0ull) | (w == (nbytes >> 6) ? 1ull << (nbytes & 63) : 0ull);
        simt::sync();            // the bytes and the bitmap: plain stores of this workgroup, read by it behind the barrier (as k_small's phases are ordered)
        stamp();
        // ---- 4. units of every byte (k_u8_len) ----
        const int nt8 = (nbytes + kU8Tile - 1) / kU8Tile;
        for (int t = wave; t < nt8; t += nwaves) {
            TkzU8Lane U;
            const int sum = tkz_u8_lane(A.d_bytes, nbytes, A.d_docbits, nwords, t, &U);
            int tot;
            (void)tkz_wave_scan_sum(sum, &tot);
            if (lane == 0) s_sum[t] = tot;
        }
        stamp();
        // ---- 5. scan, 6. the units (k_u8_write) ----
        tkz_dec_small_scan(s_sum, s_base, nt8);
        stamp();
        uint16_t* const out16 = static_cast<uint16_t*>(A.h_out);
        uint16_t* const st16 = reinterpret_cast<uint16_t*>(st);
        for (int t = wave; t < nt8; t += nwaves) {
            TkzU8Lane U;
            const int sum = tkz_u8_lane(A.d_bytes, nbytes, A.d_docbits, nwords, t, &U);
            int tot;
            const int pos = tkz_wave_scan_sum(sum, &tot);
            if (tot > kU8Stage) continue;                         // (cannot be: a tile yields at most kU8Tile + 1 units)
            tkz_u8_stage(U, nbytes, t, pos, st16);
            (void)simt::ballot(true);
            uint16_t* const dst = out16 + s_base[t];              // (units <= bytes <= kDecSmallMaxBytes, the block's capacity in units)
            for (int i = lane; i < tot; i += 64) dst[i] = st16[i];
            (void)simt::ballot(true);
        }
        stamp();
        if (tid == 0) A.h_result[2] = s_base[nt8];
    } else stamp();
    if (tid == 0) { A.h_result[1] = nbytes; A.h_result[0] = 0; }
}

// =================================================================================================
// launchers
// =================================================================================================
static inline void hook(const Launch& L, int id, int phase) { if (L.hook) L.hook(L.hook_ctx, id, phase, L.stream); }
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// a launch needs one workgroup at least (a grid of 0 is an invalid configuration on HIP; the kernels return at once for items beyond their count):
// an empty chunk of a host batch -- a UTF-16 document that spans a chunk cut -- has no tiles at all
static inline int64_t grid1(int64_t g) { return g < 1 ? 1 : g; }
static inline int64_t xcd_grid(int64_t blocks) { return (blocks + 7) & ~(int64_t)7; }     // tkz_xcd_block: XCD x takes the x-th eighth of the blocks
static inline int64_t grid_for(int64_t items) { const int64_t g = cdiv(items, kThreads); return g < 1 ? 1 : (g > 16384 ? 16384 : g); }

void launch_docmark(const Launch& L, const int64_t* d_offs, int64_t n_items, int64_t total, uint64_t* bits, int32_t* counters, int32_t* has_empty) {
    hook(L, K_DOCMARK, 0);
    TKZ_LAUNCH(k_docmark, grid_for(n_items + 1), kThreads, L.stream, d_offs, n_items, total, bits, counters, has_empty);
    hook(L, K_DOCMARK, 1);
}
void launch_pretok_rows(const Launch& L, int pattern, const uint8_t* d_bytes, const int64_t* d_offs, int64_t n_docs, int64_t total,
                        const uint64_t* docbits, uint64_t* startbits, int64_t nrows, const uint8_t* bmp, int32_t* counters,
                        int64_t* xq, unsigned long long* xcount) {
    const int64_t grid = cdiv(nrows, kRowsPerWave);           // one 64-lane workgroup per chunk of rows
    hook(L, K_PRETOK, 0);
    if (pattern == TKZ_PAT_P1)
        TKZ_LAUNCH(k_pretok_rows<TKZ_PAT_P1>, grid, 64, L.stream, d_bytes, total, docbits, startbits, nrows, bmp, counters, xq, xcount);
    else if (pattern == TKZ_PAT_CL100K)
        TKZ_LAUNCH(k_pretok_rows<TKZ_PAT_CL100K>, grid, 64, L.stream, d_bytes, total, docbits, startbits, nrows, bmp, counters, xq, xcount);
    else {
        TKZ_LAUNCH(k_pretok_rows<TKZ_PAT_O200K>, grid, 64, L.stream, d_bytes, total, docbits, startbits, nrows, bmp, counters, xq, xcount);
        // blocks with multi-byte chars: the char-level block evaluator; what that refuses as well: the sequential matcher
        int64_t* xq2 = xq + grid + 1;
        unsigned long long* xcount2 = xcount + 1;
        TKZ_LAUNCH(k_pretok_mb_blocks, grid < 8192 ? grid : 8192, 64, L.stream, d_bytes, total, docbits, startbits, nrows, bmp, (const uint8_t*)xq, grid,
                   xcount, xq2, xcount2, (int)(pattern == TKZ_PAT_O200K));
        TKZ_LAUNCH(k_pretok_seq_blocks, grid_for(n_docs > grid ? n_docs : grid), kThreads, L.stream, d_bytes, d_offs, n_docs, total, startbits, nrows,
                   pattern, bmp, (const int64_t*)xq2, (const unsigned long long*)xcount2, counters);
    }
    hook(L, K_PRETOK, 1);
}
void launch_pretok_seq(const Launch& L, int pattern, const uint8_t* d_bytes, const int64_t* d_offs, int64_t n_docs, int64_t total,
                       uint64_t* startbits, const uint8_t* bmp, int32_t* counters) {
    hook(L, K_PRETOK, 0);
    TKZ_LAUNCH(k_pretok_seq, grid_for(n_docs), kThreads, L.stream, d_bytes, d_offs, n_docs, total, startbits, pattern, bmp, counters);
    hook(L, K_PRETOK, 1);
}
// giant pieces (queued by k_list_stats): ordered, merged (k_giant_merge takes pieces off the ordered queue and exits at once when it is empty)
static void launch_giants(const Launch& L, const TkzTables& T, const EncodeParams& P) {
#ifdef TKZ_HOSTEMU
    constexpr int kGiantGrid = 2;       // (the CPU emulator pays for every thread of an idle workgroup)
#else
    constexpr int kGiantGrid = 256;
#endif
    TKZ_LAUNCH(k_giant_order, 1, 1024, L.stream, P);
    TKZ_LAUNCH(k_giant_merge, kGiantGrid, 1024, L.stream, T, P);
}
// a large batch's long misses of 17..lane_piece bytes binned by length class: the class queue k_merge_long_q takes them off
static void launch_long_queue(const Launch& L, const EncodeParams& P, int64_t nsub) {
    const int64_t nchunks = cdiv(nsub, 64), g4 = cdiv(nchunks, 4);
    TKZ_LAUNCH(k_long_count, g4 < 4096 ? g4 : 4096, kThreads, L.stream, P);
    launch_scan2(L, nchunks * kLenClasses, P.lq_bsum, P.lq_cnt, P.lq_base, P.lq_total, 1, nullptr, nullptr, nullptr, 1, -1);
    TKZ_LAUNCH(k_long_scatter, g4 < 4096 ? g4 : 4096, kThreads, L.stream, P);
}
// ... merged off the queue 256 at a time by at most `cap` wavefronts
static void launch_long_q(hipStream_t st, const TkzTables& T, const EncodeParams& P, int64_t cap) {
    const int64_t ranges = cdiv(P.lq_cap, kLqRangeLong), grid = ranges < cap ? (ranges < 1 ? 1 : ranges) : cap;
    if (T.max_rank <= kVarCompactMaxRank) TKZ_LAUNCH((k_merge_long_q<true>), grid, 64, st, T, P);
    else TKZ_LAUNCH((k_merge_long_q<false>), grid, 64, st, T, P);
}
// the pieces the lane mergers leave to a whole wavefront, off the queue k_list_stats filled (every wavefront exits at once when it is empty)
static void launch_coop(hipStream_t st, const TkzTables& T, const EncodeParams& P, int64_t grid, int64_t cap) {
    TKZ_LAUNCH(k_merge_coop, grid < cap ? grid : cap, 64, st, T, P);
}
// grids of the two tail kernels beside k_merge_short: they fit the chip beside each other and leave k_merge_short the rest
constexpr int64_t kSideLongGrid = 2048, kSideCoopGrid = 1024;
void launch_encode(const Launch& L, const TkzTables& T, const EncodeParams& P, int64_t nsub) {
    hook(L, K_ENCODE, 0);
    if (P.specbits) TKZ_LAUNCH(k_probe_special, xcd_grid(cdiv(nsub, (kThreads / 64) * kProbePer)), kThreads, L.stream, T, P);
    else TKZ_LAUNCH(k_probe, xcd_grid(cdiv(nsub, (kThreads / 64) * kProbePer)), kThreads, L.stream, T, P);
    hook(L, K_ENCODE, 1);
    // (the list statistics and, in the same pass, the giant pieces of the sub-tiles k_probe flagged: queued for k_giant_order / k_giant_merge)
    { const int64_t g = grid_for(nsub); TKZ_LAUNCH(k_list_stats, g < 1024 ? g : 1024, kThreads, L.stream, (const uint32_t*)P.mcount, nsub, P.mcap, P.counters,
                                                     (const uint8_t*)P.heavy_flag, P.startbits, P.nwords, P.total, P.giant_q, P.giant_count, P.giant_cap,
                                                     (const uint32_t*)P.mlist, P.coop_q, P.coop_count, P.coop_cap, (int)P.lane_piece, P.miss_sums); }
    const int64_t nb_short = xcd_grid(cdiv(nsub, (kMsThreads / 64) * kGroup));     // (workgroups of k_merge_short)
    if (P.latency) {
        // A SMALL batch (its token counts are summed with atomics: P.tc_atomic): the giant pieces, then the three merge stages as one launch -- k_merge_latency.
        // A small batch gets as many k_merge_coop wavefronts as a large one: 16 of them took 107 us over the queue of a 1 MB call.
        hook(L, K_HEAVY, 0);
        launch_giants(L, T, P);
        hook(L, K_HEAVY, 1);
        const int64_t chunks = cdiv(nsub, 64) * kLongPartsLatency, nb_long = cdiv(chunks < 65536 ? chunks : 65536, kMsThreads / 64);
        hook(L, K_MERGE_SHORT, 0);
        if (T.max_rank <= kVarCompactMaxRank) TKZ_LAUNCH((k_merge_latency<true>), nb_short + nb_long, kMsThreads, L.stream, T, P, (int)nb_short, (int)nb_long);
        else TKZ_LAUNCH((k_merge_latency<false>), nb_short + nb_long, kMsThreads, L.stream, T, P, (int)nb_short, (int)nb_long);
        // (the queue of the 129+-byte pieces stays a launch of its own BEHIND the chunk form of the long lists, as it always was: inside the same launch its pieces came
        //  out wrong on the GPU -- test_pieces_vs_oracle_bpe, test_mid_pieces_share_the_arena -- while the emulator, whose workgroups take turns, saw nothing)
        launch_coop(L.stream, T, P, 512, kCoopGrid);
        hook(L, K_MERGE_SHORT, 1);
    } else if (!L.side) {
        // a large batch, serial: k_merge_short in front, as it always was, then the giant pieces, the class queue and the long misses
        hook(L, K_MERGE_SHORT, 0);
        TKZ_LAUNCH(k_merge_short, nb_short, kMsThreads, L.stream, T, P);
        hook(L, K_MERGE_SHORT, 1);
        hook(L, K_HEAVY, 0);
        launch_giants(L, T, P);
        launch_long_queue(L, P, nsub);
        launch_long_q(L.stream, T, P, kLongQGrid);
        launch_coop(L.stream, T, P, cdiv(nsub, 64), kCoopGrid);
        hook(L, K_HEAVY, 1);
    } else {
        // a large batch, side by side (L.side: P.tc_atomic).  The short misses and the long ones touch different list entries and the sub-tiles' token counts are
        // summed with atomics from zero, so the kernels of the two kinds may run side by side.  What makes that worth having: k_merge_long_q and k_merge_coop last as
        // long as their slowest wavefronts, not as long as their work (0.43 + 0.31 of the 3.7 ms of a 268 MB batch of real text, for 0.6 M pieces), while
        // k_merge_short keeps the whole chip busy.
        // How: this chip starts no workgroup of a second kernel while a first one still has workgroups waiting (tools/stream_overlap_probe.hip: 8,192 + 64 workgroups
        // on two streams take 20 + 5 ms whatever the streams' priorities; 1,024 + 64 take 5) -- so the two tail kernels go FIRST, each on a stream of its own with a
        // grid that fits the chip beside the other, and k_merge_short behind them on L.stream takes what is left and, as their wavefronts retire, everything.
        // The giant pieces and the counting, the scan and the scatter of the class queue stay in front on L.stream (they are short and the queue kernel needs them).
        // (k_merge_coop ALONE beside k_merge_short, for workspaces whose class queue is long, was measured too: mixed text 15.97 -> 15.87 ms, headline 20.59 -> 20.84 -- not kept.)
        hook(L, K_HEAVY, 0);
        launch_giants(L, T, P);
        launch_long_queue(L, P, nsub);
        hook(L, K_HEAVY, 1);            // (the bracket of this form: what runs in front of the three; K_MERGE_SHORT's is the three side by side)
        hook(L, K_MERGE_SHORT, 0);
        (void)hipEventRecord(L.ev_fork, L.stream); (void)hipStreamWaitEvent(L.side, L.ev_fork, 0); (void)hipStreamWaitEvent(L.side2, L.ev_fork, 0);
        launch_long_q(L.side, T, P, kSideLongGrid);
        launch_coop(L.side2, T, P, cdiv(nsub, 64), kSideCoopGrid);
        (void)hipEventRecord(L.ev_join, L.side); (void)hipEventRecord(L.ev_join2, L.side2);
        TKZ_LAUNCH(k_merge_short, nb_short, kMsThreads, L.stream, T, P);
        (void)hipStreamWaitEvent(L.stream, L.ev_join, 0); (void)hipStreamWaitEvent(L.stream, L.ev_join2, 0);
        hook(L, K_MERGE_SHORT, 1);
    }
}
// k_probe and the list statistics over the first `nsample` sub-tiles only (tkz_api.cpp: the sizing attempt of a fresh workspace)
void launch_probe_sample(const Launch& L, const TkzTables& T, const EncodeParams& P, int64_t nsample) {
    if (nsample > P.nsub) nsample = P.nsub;
    hook(L, K_ENCODE, 0);
    if (P.specbits) TKZ_LAUNCH(k_probe_special, xcd_grid(cdiv(nsample, (kThreads / 64) * kProbePer)), kThreads, L.stream, T, P);
    else TKZ_LAUNCH(k_probe, xcd_grid(cdiv(nsample, (kThreads / 64) * kProbePer)), kThreads, L.stream, T, P);
    hook(L, K_ENCODE, 1);
    { const int64_t g = grid_for(nsample); TKZ_LAUNCH(k_list_stats, g < 1024 ? g : 1024, kThreads, L.stream, (const uint32_t*)P.mcount, nsample, P.mcap, P.counters,
                                                     (const uint8_t*)P.heavy_flag, P.startbits, P.nwords, P.total, P.giant_q, P.giant_count, P.giant_cap,
                                                     (const uint32_t*)P.mlist, P.coop_q, P.coop_count, P.coop_cap, (int)P.lane_piece, P.miss_sums); }
}
void launch_ingest(const Launch& L, const uint8_t* h_bytes, int64_t total, uint8_t* d_bytes, const int64_t* h_offs, int64_t n_offs, int64_t* d_offs, void* zero, int64_t zero_bytes) {
    const int64_t quads = std::max<int64_t>(total / 16 + 1, (zero_bytes + 15) / 16);
    const int64_t g = cdiv(quads, kThreads * 4);               // (four quads a thread: ~64 loads over PCIe in flight per wavefront is what fills the link)
    TKZ_LAUNCH(k_ingest, g < 1 ? 1 : (g > 2048 ? 2048 : g), kThreads, L.stream, h_bytes, total, d_bytes, h_offs, n_offs, d_offs, reinterpret_cast<uint4*>(zero), (zero_bytes + 15) / 16);
}
void launch_small(const Launch& L, const TkzTables& T, const EncodeParams& P, const SmallArgs& A) {
    if (A.trim && A.n_taken) TKZ_LAUNCH((k_small<true, true>), 1, P.nsub <= 4 ? 256 : 1024, L.stream, T, P, A);
    else if (A.trim) TKZ_LAUNCH((k_small<false, true>), 1, P.nsub <= 4 ? 256 : 1024, L.stream, T, P, A);
    else if (A.n_taken) TKZ_LAUNCH(k_small<true>, 1, P.nsub <= 4 ? 256 : 1024, L.stream, T, P, A);
    else TKZ_LAUNCH(k_small<false>, 1, P.nsub <= 4 ? 256 : 1024, L.stream, T, P, A);
}
void launch_dec_small(const Launch& L, const TkzDecodeTable& D, const DecSmallArgs& A) {
    const int block = A.n_ids <= 4 * kDecTile ? 256 : 1024;
    if (A.utf16) TKZ_LAUNCH(k_dec_small<true>, 1, block, L.stream, D, A);
    else TKZ_LAUNCH(k_dec_small<false>, 1, block, L.stream, D, A);
}
void launch_place(const Launch& L, const EncodeParams& P, const int64_t* tile_base, int64_t nsub, int32_t* out, int64_t out_cap) {
    hook(L, K_GATHER, 0);
    const int64_t grid = xcd_grid(cdiv(nsub, (kThreads / 64) * kPlacePer));
    if (P.promo) {      // (promoted pieces in the tables: the records may carry promo codes)
        if (P.place128) TKZ_LAUNCH((k_place<128, true>), grid, kThreads, L.stream, P, tile_base, out, out_cap);
        else TKZ_LAUNCH((k_place<64, true>), grid, kThreads, L.stream, P, tile_base, out, out_cap);
    } else {
        if (P.place128) TKZ_LAUNCH((k_place<128, false>), grid, kThreads, L.stream, P, tile_base, out, out_cap);
        else TKZ_LAUNCH((k_place<64, false>), grid, kThreads, L.stream, P, tile_base, out, out_cap);
    }
    hook(L, K_GATHER, 1);
}
// the count form of launch_place, in the same profiling bracket (tile_base: the positions k_tokcount writes are relative to their sub-tile -- k_docoffs adds the
// base --, so the kernel does not read it; the argument keeps the two launchers interchangeable where the launch sequence chooses between them)
void launch_tokcount(const Launch& L, const EncodeParams& P, const int64_t* tile_base, const int32_t* dcount, int64_t nsub) {
    (void)tile_base;
    hook(L, K_GATHER, 0);
    TKZ_LAUNCH(k_tokcount, xcd_grid(cdiv(nsub, (kThreads / 64) * kPlacePer)), kThreads, L.stream, P, dcount);
    hook(L, K_GATHER, 1);
}
void launch_doccount2(const Launch& L, const uint64_t* bits_a, const uint64_t* bits_b, int64_t nwords, int64_t total, int64_t nsub, int32_t* cnt_a, int32_t* cnt_b) {
    TKZ_LAUNCH(k_doccount2, grid_for(nsub * (kSub / 64)), kThreads, L.stream, bits_a, bits_b, nwords, total, nsub, cnt_a, cnt_b);
}
void launch_scan2(const Launch& L, int64_t ntiles, int64_t* bsum, const int32_t* cnt_a, int64_t* base_a, int64_t* grand_a, int round_to_a,
                  const int32_t* cnt_b, int64_t* base_b, int64_t* grand_b, int round_to_b, int kid) {
    if (ntiles <= kScanSmallMax) {
        if (kid >= 0) hook(L, kid, 0);
        TKZ_LAUNCH(k_scan_small, 1, 1024, L.stream, cnt_a, base_a, grand_a, round_to_a > 1 ? round_to_a - 1 : 0, cnt_b, base_b, grand_b, round_to_b > 1 ? round_to_b - 1 : 0, (int)ntiles);
        if (kid >= 0) hook(L, kid, 1);
        return;
    }
    launch_scan(L, cnt_a, ntiles, bsum, base_a, grand_a, kid, round_to_a);
    if (cnt_b) launch_scan(L, cnt_b, ntiles, bsum, base_b, grand_b, kid, round_to_b);
}
void launch_scan(const Launch& L, const int32_t* tile_count, int64_t ntiles, int64_t* bsum, int64_t* tile_base, int64_t* grand, int kid, int round_to) {
    const int64_t nblk = grid1(cdiv(ntiles, kScanBlock));     // (no tiles: one workgroup that writes a zero sum)
    const int round = round_to > 1 ? round_to - 1 : 0;       // (round_to: a power of two)
    if (kid >= 0) hook(L, kid, 0);
    TKZ_LAUNCH(k_scan_partials, nblk, kThreads, L.stream, tile_count, ntiles, bsum, round);
    TKZ_LAUNCH(k_scan_top, 1, kThreads, L.stream, bsum, nblk, grand);
    TKZ_LAUNCH(k_scan_final, nblk, kThreads, L.stream, tile_count, ntiles, (const int64_t*)bsum, tile_base, round);
    if (kid >= 0) hook(L, kid, 1);
}
void launch_docoffs(const Launch& L, const int64_t* d_offs, int64_t n_docs, int64_t total, const int64_t* tile_base,
                    const uint64_t* docbits, const int64_t* docord_base, const int32_t* doc_tok, const int64_t* grand, int64_t* out_offs,
                    const int32_t* has_empty, int64_t c3_docs, int64_t* c3a, int64_t* c3b, int64_t* c3c) {
    hook(L, K_DOCOFFS, 0);
    TKZ_LAUNCH(k_docoffs, grid_for(n_docs + 1), kThreads, L.stream, d_offs, n_docs, total, tile_base, docbits, docord_base, doc_tok, grand, out_offs, c3_docs, c3a, c3b, c3c, has_empty);
    hook(L, K_DOCOFFS, 1);
}
void launch_case_equiv_fix(const Launch& L, const uint8_t* d_bytes, int64_t total, const uint64_t* docbits, uint64_t* startbits) {
    TKZ_LAUNCH(k_case_equiv_fix, grid_for((total + 7) / 8), kThreads, L.stream, d_bytes, total, docbits, startbits);
}
// (the brackets: the scan and the segment bitmap extend K_DOCMARK's, the fix-up K_PRETOK's -- the closing event is recorded again behind them)
void launch_lit_scan(const Launch& L, const uint8_t* d_bytes, int64_t total, const uint64_t* docbits, int64_t nwords, const TkzLitTable& LT, const TkzLitAllowed& A,
                     uint64_t* candbits, uint64_t* segbits, uint64_t* specbits, uint64_t* endbits, unsigned long long* n_taken, const uint64_t* repl) {
    TKZ_LAUNCH(k_lit_scan, grid1(cdiv(nwords, (kThreads / 64) * (kLitBlock / 64))), kThreads, L.stream, d_bytes, total, docbits, nwords, LT, A, candbits, segbits, specbits, endbits, repl);
    TKZ_LAUNCH(k_lit_resolve, grid_for(nwords), kThreads, L.stream, d_bytes, total, docbits, (const uint64_t*)candbits, nwords, LT, segbits, specbits, endbits, n_taken, repl);
    hook(L, K_DOCMARK, 1);
}
void launch_lit_fix(const Launch& L, uint64_t* startbits, const uint64_t* segbits, const uint64_t* specbits, const uint64_t* endbits, int64_t nwords) {
    TKZ_LAUNCH(k_lit_fix, grid_for(nwords), kThreads, L.stream, startbits, segbits, specbits, endbits, nwords);
    hook(L, K_PRETOK, 1);
}
void launch_seg_offsets(const Launch& L, const uint64_t* segbits, int64_t nwords, int64_t total, int64_t nsub, const int64_t* ord_base, int64_t n_seg, int64_t* seg_offs) {
    TKZ_LAUNCH(k_piece_index, grid1(cdiv(nsub, kThreads / 64)), kThreads, L.stream, segbits, nwords, total, nsub, ord_base, n_seg, seg_offs);
}
void launch_rebase(const Launch& L, int64_t* offs, int64_t n, int64_t base) {
    TKZ_LAUNCH(k_rebase, grid_for(n), kThreads, L.stream, offs, n, base);
}
void launch_miss_stats(const Launch& L, const EncodeParams& P, int64_t nsub) {
    const int64_t g = grid_for(nsub);
    TKZ_LAUNCH(k_miss_stats, g < 1024 ? g : 1024, kThreads, L.stream, (const uint32_t*)P.mcount, P.pcount, nsub, P.stats);
}
void launch_counts3(const Launch& L, int64_t n_docs, int64_t total, const int64_t* grand, int64_t* out3, int64_t* out3b, int64_t* out3c) {
    TKZ_LAUNCH(k_counts3, 1, 64, L.stream, n_docs, total, grand, out3, out3b, out3c);
}
void launch_u16_len(const Launch& L, const uint16_t* units, int64_t total, const uint64_t* docbits, int64_t ntiles, int32_t* grp_prefix, int32_t* tile_sum) {
    TKZ_LAUNCH(k_u16_len, grid1(cdiv(ntiles, kThreads / 64)), kThreads, L.stream, units, total, docbits, ntiles, grp_prefix, tile_sum);
}
void launch_u16_write(const Launch& L, const uint16_t* units, int64_t total, const uint64_t* docbits, int64_t ntiles, const int64_t* tile_base,
                      uint8_t* out, const int64_t* unit_offs, int64_t n_docs, const int32_t* grp_prefix, const int64_t* grand, int64_t* byte_offs, uint64_t* repl) {
    TKZ_LAUNCH(k_u16_write, grid1(cdiv(ntiles, kThreads / 64)), kThreads, L.stream, units, total, docbits, ntiles, tile_base, out, repl);
    TKZ_LAUNCH(k_u16_docoffs, grid_for(n_docs + 1), kThreads, L.stream, units, total, docbits, unit_offs, n_docs, tile_base, grp_prefix, grand, byte_offs);
}
int64_t u16_tiles(int64_t total_units) { return cdiv(total_units, kU16Tile); }
void launch_piece_index(const Launch& L, const uint64_t* startbits, int64_t nwords, int64_t total, int64_t nsub, const int64_t* ord_base,
                        int64_t n_pieces, int64_t* piece_offs, const int64_t* d_offs, int64_t n_docs, int64_t* doc_piece) {
    TKZ_LAUNCH(k_piece_index, grid1(cdiv(nsub, kThreads / 64)), kThreads, L.stream, startbits, nwords, total, nsub, ord_base, n_pieces, piece_offs);
    TKZ_LAUNCH(k_doc_piece, grid_for(n_docs + 1), kThreads, L.stream, d_offs, n_docs, total, startbits, ord_base, n_pieces, doc_piece);
}
// (outside the profiling brackets, like k_list_stats: tkz.h at tkz_encoder_set_profiling)
void launch_trim(const Launch& L, const TrimParams& R, const int32_t* ids, int64_t ids_cap, int32_t* out, int64_t out_cap, int64_t* out_offs, int64_t* kept_total) {
    TKZ_LAUNCH(k_trim_cut, grid_for(R.n_docs), kThreads, L.stream, R);
    const int64_t nblk = grid1(cdiv(R.n_docs, kScanBlock));
    TKZ_LAUNCH(k_scan_partials64, nblk, kThreads, L.stream, (const int64_t*)R.keep_n, R.n_docs, R.bsum);
    TKZ_LAUNCH(k_scan_top, 1, kThreads, L.stream, R.bsum, nblk, out_offs + R.n_docs);
    TKZ_LAUNCH(k_scan_final64, nblk, kThreads, L.stream, (const int64_t*)R.keep_n, R.n_docs, (const int64_t*)R.bsum, out_offs);
    // (a wavefront per tile of the larger of the two ranges -- the kept ids are at most the bytes --, grid-strided beyond 2,048 workgroups)
    const int64_t tiles = cdiv(R.total, kTrimTile), g = cdiv(tiles, kThreads / 64);
    TKZ_LAUNCH(k_trim_gather, g < 1 ? 1 : (g > 2048 ? 2048 : g), kThreads, L.stream, R, ids, ids_cap, (const int64_t*)out_offs, out, out_cap, kept_total);
}
// (the bracket: the stage extends K_DOCOFFS's -- the closing event is recorded again behind it, as launch_lit_fix does for K_PRETOK)
void launch_tokspans(const Launch& L, const SpanParams& S, const TkzDecodeTable& D) {
    TKZ_LAUNCH(k_tokspan_mark, grid_for(S.n_pieces > S.n_docs ? S.n_pieces : S.n_docs + 1), kThreads, L.stream, S, D);
    const int64_t g = grid1(cdiv(S.nsub, kThreads / 64));
    TKZ_LAUNCH(k_tokspan_count, g, kThreads, L.stream, S);
    launch_scan2(L, S.nsub, S.bsum, S.cnt_tok, S.base_tok, S.sums, 1, S.tok_units ? S.cnt_unit : nullptr, S.base_unit, S.sums + 1, 1, -1);
    TKZ_LAUNCH(k_tokspan_write, g, kThreads, L.stream, S);
    hook(L, K_DOCOFFS, 1);
}
// (the bracket: K_DOCOFFS's again.  How many documents are listed and how many chunks there are is known on the device only: the wavefront kernels get a grid
//  that the bounds allow -- a listed document has more than kChunkLongItems bytes, chunk_cap chunks at most are written -- and stride over what there is)
void launch_chunks(const Launch& L, const ChunkParams& C, const TkzDecodeTable& D) {
    const int64_t g_docs = grid_for(C.n_docs + 1), nblk = grid1(cdiv(C.n_docs, kScanBlock));
    int64_t g_long = cdiv(C.total / kChunkLongItems, kThreads / 64), g_units = cdiv(cdiv(C.chunk_cap, 64), kThreads / 64);
    g_long = g_long < 1 ? 1 : (g_long > 1024 ? 1024 : g_long);
    g_units = g_units < 1 ? 1 : (g_units > 2048 ? 2048 : g_units);
    TKZ_LAUNCH(k_chunk_walk, g_docs, kThreads, L.stream, C, D, 0);
    TKZ_LAUNCH(k_chunk_walk_long, g_long, kThreads, L.stream, C, D, 0);
    TKZ_LAUNCH(k_scan_partials64, nblk, kThreads, L.stream, (const int64_t*)C.doc_cnt, C.n_docs, C.bsum);
    TKZ_LAUNCH(k_scan_top, 1, kThreads, L.stream, C.bsum, nblk, C.doc_chunk_offs + C.n_docs);
    TKZ_LAUNCH(k_scan_final64, nblk, kThreads, L.stream, (const int64_t*)C.doc_cnt, C.n_docs, (const int64_t*)C.bsum, C.doc_chunk_offs);
    if (C.chunk_units) {
        TKZ_LAUNCH(k_chunk_unitcount, grid1(cdiv(cdiv(C.total, kSub), kThreads / 64)), kThreads, L.stream, C);
        launch_scan(L, C.cnt_unit, C.nspan, C.ubsum, C.base_unit, C.usum, -1, 1);
    }
    TKZ_LAUNCH(k_chunk_walk, g_docs, kThreads, L.stream, C, D, 1);
    TKZ_LAUNCH(k_chunk_walk_long, g_long, kThreads, L.stream, C, D, 1);
    if (C.chunk_units) TKZ_LAUNCH(k_chunk_units, g_units, kThreads, L.stream, C);
    hook(L, K_DOCOFFS, 1);
}
// (launch_chunks' sequence and grids with the overlap walks; the unit stage runs for either unit array)
void launch_chunks_overlap(const Launch& L, const ChunkOvParams& V, const TkzDecodeTable& D) {
    const ChunkParams& C = V.C;
    const int64_t g_docs = grid_for(C.n_docs + 1), nblk = grid1(cdiv(C.n_docs, kScanBlock));
    int64_t g_long = cdiv(C.total / kChunkLongItems, kThreads / 64), g_units = cdiv(cdiv(C.chunk_cap, 64), kThreads / 64);
    g_long = g_long < 1 ? 1 : (g_long > 1024 ? 1024 : g_long);
    g_units = g_units < 1 ? 1 : (g_units > 2048 ? 2048 : g_units);
    const bool units = C.chunk_units || V.chunk_end_units;
    TKZ_LAUNCH(k_chunkov_walk, g_docs, kThreads, L.stream, V, D, 0);
    TKZ_LAUNCH(k_chunkov_walk_long, g_long, kThreads, L.stream, V, D, 0);
    TKZ_LAUNCH(k_scan_partials64, nblk, kThreads, L.stream, (const int64_t*)C.doc_cnt, C.n_docs, C.bsum);
    TKZ_LAUNCH(k_scan_top, 1, kThreads, L.stream, C.bsum, nblk, C.doc_chunk_offs + C.n_docs);
    TKZ_LAUNCH(k_scan_final64, nblk, kThreads, L.stream, (const int64_t*)C.doc_cnt, C.n_docs, (const int64_t*)C.bsum, C.doc_chunk_offs);
    if (units) {
        TKZ_LAUNCH(k_chunk_unitcount, grid1(cdiv(cdiv(C.total, kSub), kThreads / 64)), kThreads, L.stream, C);
        launch_scan(L, C.cnt_unit, C.nspan, C.ubsum, C.base_unit, C.usum, -1, 1);
    }
    TKZ_LAUNCH(k_chunkov_walk, g_docs, kThreads, L.stream, V, D, 1);
    TKZ_LAUNCH(k_chunkov_walk_long, g_long, kThreads, L.stream, V, D, 1);
    if (units) TKZ_LAUNCH(k_chunkov_units, g_units, kThreads, L.stream, V);
    hook(L, K_DOCOFFS, 1);
}
// (the bracket: K_DOCOFFS's again.  How long the stream is is known on the device only: the counting grid is sized for the tiles the bound allows, the writing
//  grid for the rows that fit the caller's buffer -- beyond kPackGridMax workgroups both stride)
void launch_pack(const Launch& L, const PackParams& K) {
    const int64_t waves = kThreads / 64, g_count = cdiv(K.ntile, waves), g_write = cdiv(cdiv(K.out_cap, kPackTile), waves);
    const auto capped = [](int64_t g) { return g < 1 ? 1 : (g > kPackGridMax ? kPackGridMax : g); };
    TKZ_LAUNCH(k_pack_count, capped(g_count), kThreads, L.stream, K);
    launch_scan(L, K.cnt, K.ntile, K.bsum, K.base, K.totals + 2, -1, 1);
    TKZ_LAUNCH(k_pack_write, capped(g_write > g_count ? g_write : g_count), kThreads, L.stream, K);
    hook(L, K_DOCOFFS, 1);
}
int64_t dec_tiles(int64_t total_ids) { return cdiv(total_ids, kDecTile); }
void launch_dec_len(const Launch& L, const TkzDecodeTable& D, const int32_t* ids, int64_t total, int64_t ntiles, int32_t* grp_prefix, int32_t* tile_sum) {
    TKZ_LAUNCH(k_dec_len, grid1(cdiv(ntiles, kThreads / 64)), kThreads, L.stream, D, ids, total, ntiles, grp_prefix, tile_sum);
}
void launch_dec_write(const Launch& L, const TkzDecodeTable& D, const int32_t* ids, int64_t total, int64_t ntiles, const int64_t* tile_base, uint8_t* out,
                      int64_t out_cap, const int64_t* id_offs, int64_t n_docs, const int32_t* grp_prefix, const int64_t* grand, int64_t* byte_offs, int32_t* counters) {
    TKZ_LAUNCH(k_dec_write, grid1(cdiv(ntiles, kThreads / 64)), kThreads, L.stream, D, ids, total, ntiles, tile_base, out, out_cap);
    TKZ_LAUNCH(k_dec_docoffs, grid_for(n_docs + 1), kThreads, L.stream, D, ids, total, id_offs, n_docs, tile_base, grp_prefix, grand, byte_offs, counters);
}
int64_t u8_tiles(int64_t total_bytes) { return cdiv(total_bytes, kU8Tile); }
void launch_u8_len(const Launch& L, const uint8_t* bytes, int64_t total, const uint64_t* docbits, int64_t nwords, int64_t ntiles, int32_t* grp_prefix, int32_t* tile_sum) {
    TKZ_LAUNCH(k_u8_len, grid1(cdiv(ntiles, kThreads / 64)), kThreads, L.stream, bytes, total, docbits, nwords, ntiles, grp_prefix, tile_sum);
}
void launch_u8_write(const Launch& L, const uint8_t* bytes, int64_t total, const uint64_t* docbits, int64_t nwords, int64_t ntiles, const int64_t* tile_base,
                     uint16_t* out, int64_t out_cap, const int64_t* byte_offs, int64_t n_docs, const int32_t* grp_prefix, const int64_t* grand, int64_t* unit_offs) {
    TKZ_LAUNCH(k_u8_write, grid1(cdiv(ntiles, kThreads / 64)), kThreads, L.stream, bytes, total, docbits, nwords, ntiles, tile_base, out, out_cap);
    TKZ_LAUNCH(k_u8_docoffs, grid_for(n_docs + 1), kThreads, L.stream, bytes, total, docbits, nwords, byte_offs, n_docs, tile_base, grp_prefix, grand, unit_offs);
}
void launch_corpus(hipStream_t s, int kind, uint64_t seed, int64_t first_doc, int64_t n_docs, int min_len, int max_len,
                   int64_t* d_offs, uint8_t* d_bytes, int64_t cap_bytes, int64_t* d_total) {
    TKZ_LAUNCH(k_corpus_lengths, grid_for(n_docs), kThreads, s, kind, seed, first_doc, n_docs, min_len, max_len, d_offs);
    TKZ_LAUNCH(k_offsets_scan, 1, kThreads, s, d_offs, n_docs, d_total);
    TKZ_LAUNCH(k_corpus_fill, grid_for(n_docs), kThreads, s, kind, seed, first_doc, n_docs, min_len, max_len,
               (const int64_t*)d_offs, d_bytes, cap_bytes);
}

// -------------------------------------------------------------------------------------------------
// Pair rows (tkz_encode_batch_pairs_device; tkz.h states the rule), behind the plain document-granular launch sequence: documents 2p and 2p + 1 are the two
// texts A and B of pair p, and row p is [bos] A-kept sep x s B-kept [eos], cut to max_len as a whole, padded to the common width W on either side, with the mask,
// the type of every position and the position inside the content.  The uncut ids and offsets O stay in the workspace.
//   k_pair_lens   a lane a pair: a = O[2p + 1] - O[2p], b = O[2p + 2] - O[2p + 1], R = L - f, h = R / 2, H = R - h.  The kept counts in closed form --
//                 LONGEST_FIRST ka = min(a, max(H, R - b)), kb = min(b, max(h, R - a)); ONLY_FIRST kb = min(b, R), ka = min(a, R - kb); ONLY_SECOND ka = min(a, R),
//                 kb = min(b, R - ka) --, lens[p] = ka + kb + f, the row's RECORD of 24 bytes in the workspace -- srcA, srcB = the index of the first kept id of
//                 either text (the head, or the tail for a cut at the front), and {len, ka} in one word --, and the caller's kept and out_offs.  The largest len and the number of cut pairs of a workgroup go into ONE partial each,
//                 as k_pad_lens makes its own: the wavefronts' by shuffles, the four of them through 48 bytes of LDS.  Nothing is added up in memory, so the
//                 result is the same bytes on every run.
//   k_pair_write  k_pad_write's frame: every wavefront reduces the partials to W and n_cut, one lane stores {total, W, n_cut}, n_pairs * W is held against
//                 out_cap here, and the rows are dealt out by OUTPUT position, a wavefront per tile of kPairTile positions, grid-strided: one 64-bit division
//                 a TILE, additions and one conditional subtraction per group of 64 positions.  A lane loads its row's record (srcA, srcB, len, ka: 24 bytes side by
//                 side, which measured a third faster than four loads from three arrays) only when its row changes.  The index j inside the content selects the source: bos, A (srcA + j - fb), a separator, B (srcB + j - fb - ka - s), or eos;
//                 the type is j >= fb + ka + s.  It reads the records, not O or how the cut was made: whoever fills them decides what is kept.
// Every store of a row is tkz_store_nt, all 64 lanes, consecutive addresses; the ids are read with tkz_load_nt, below ids_cap.
// -------------------------------------------------------------------------------------------------
TKZ_DEV int tkz_pad_wave_max(int v);
TKZ_DEV int64_t tkz_pad_wave_sum(int64_t v);
TKZ_KERNEL(256) void k_pair_lens(PairParams K) {
    TKZ_SHARED int s_len[kThreads / 64];
    TKZ_SHARED int64_t s_cut[kThreads / 64];
    const bool bad = K.counters[0] != 0;                       // (a failed attempt: the offsets mean nothing, the caller's buffers are left alone)
    const int64_t f = (K.bos_id >= 0 ? 1 : 0) + (K.eos_id >= 0 ? 1 : 0) + K.sep_count, R = K.max_len - f, h = R / 2, H = R - h;
    const int64_t stride = simt::nblocks() * simt::nthreads();
    int longest = 0;
    int64_t ncut = 0;
    if (!bad) for (int64_t p = simt::bid() * simt::nthreads() + simt::tid(); p < K.n_pairs; p += stride) {
        const int64_t o0 = K.offs[2 * p], o1 = K.offs[2 * p + 1], o2 = K.offs[2 * p + 2], a = o1 - o0, b = o2 - o1;
        int64_t ka, kb;
        if (K.strategy == 1) { kb = b < R ? b : R; ka = a < R - kb ? a : R - kb; }                       // ONLY_FIRST: A gives way first
        else if (K.strategy == 2) { ka = a < R ? a : R; kb = b < R - ka ? b : R - ka; }                  // ONLY_SECOND
        else {                                                                                           // LONGEST_FIRST: the shorter text keeps its half at least
            const int64_t ra = R - b > H ? R - b : H, rb = R - a > h ? R - a : h;
            ka = a < ra ? a : ra; kb = b < rb ? b : rb;
        }
        const int len = (int)(ka + kb + f);
        K.lens[p] = len;
        K.rows[3 * p] = K.cut_side ? o1 - ka : o0;                 // the row's record: the first kept id of A, of B, and {len, ka} in one word
        K.rows[3 * p + 1] = K.cut_side ? o2 - kb : o1;
        K.rows[3 * p + 2] = (int64_t)((uint64_t)(uint32_t)len | ((uint64_t)(uint32_t)ka << 32));
        if (K.kept) { K.kept[2 * p] = (int32_t)ka; K.kept[2 * p + 1] = (int32_t)kb; }
        if (K.out_offs) { K.out_offs[2 * p] = o0; K.out_offs[2 * p + 1] = o1; if (p == K.n_pairs - 1) K.out_offs[2 * p + 2] = o2; }
        longest = len > longest ? len : longest;
        ncut += a + b > R ? 1 : 0;
    }
    longest = tkz_pad_wave_max(longest);
    ncut = tkz_pad_wave_sum(ncut);
    if (simt::lane() == 0) { s_len[simt::wave()] = longest; s_cut[simt::wave()] = ncut; }
    simt::sync();
    if (simt::tid() == 0) {
        int64_t c = 0;
        for (int w = 0; w < simt::nthreads() / 64; ++w) { longest = s_len[w] > longest ? s_len[w] : longest; c += s_cut[w]; }
        K.part_len[simt::bid()] = longest;
        K.part_cut[simt::bid()] = c;
    }
}
TKZ_KERNEL(256) void k_pair_write(PairParams K) {
    if (K.counters[0] != 0) return;
    const int lane = simt::lane();
    const int64_t nwaves = simt::nblocks() * (kThreads / 64), wave0 = simt::bid() * (kThreads / 64) + simt::wave();
    // the width and the cut pairs, from the partials
    int longest = 0;
    int64_t n_cut = 0;
    for (int i = lane; i < K.nparts; i += 64) {
        const int l = K.part_len[i];
        longest = l > longest ? l : longest;
        n_cut += K.part_cut[i];
    }
    longest = tkz_pad_wave_max(longest);
    n_cut = tkz_pad_wave_sum(n_cut);
    const int64_t L = K.max_len, M = K.pad_multiple;
    int64_t W = 0;
    if (longest > 0) { W = M == 0 ? L : (longest + M - 1) / M * M; W = W < L ? W : L; }
    W = (int64_t)simt::uniform64((uint64_t)W);
    if (wave0 == 0 && lane == 0) { K.totals[0] = *K.grand; K.totals[1] = W; K.totals[2] = n_cut; }
    if (W == 0 || K.n_pairs > K.out_cap / W) return;           // (nothing to write; or the rows do not fit: the totals are all that is written)
    const int64_t N = K.n_pairs * W, ntile = (N + kPairTile - 1) / kPairTile;
    const int fb = K.bos_id >= 0 ? 1 : 0, fe = K.eos_id >= 0 ? 1 : 0, ns = K.sep_count;
    // 64 positions on: rstep rows and cstep < W columns
    const int64_t rstep = W > 64 ? 0 : (int64_t)(64u / (uint32_t)W), cstep = W > 64 ? 64 : (int64_t)(64u % (uint32_t)W);
    for (int64_t t = wave0; t < ntile; t += nwaves) {
        const int64_t q0 = t * kPairTile, q1 = q0 + kPairTile < N ? q0 + kPairTile : N;
        const int64_t row0 = q0 / W, col0 = q0 - row0 * W;     // (wave-uniform: one division a tile)
        int64_t r, c;
        if (W >= 64) { r = row0; c = col0 + lane; if (c >= W) { c -= W; ++r; } }
        else { const uint32_t x = (uint32_t)col0 + (uint32_t)lane; r = row0 + (int64_t)(x / (uint32_t)W); c = (int64_t)(x % (uint32_t)W); }
        int64_t cur = -1, srcA = 0, srcB = 0;
        int len = 0, ka = 0;
        for (int64_t g = q0; g < q1; g += 64) {
            const int64_t q = g + lane;
            if (q < q1) {
                if (r != cur) {                                // (one record of 24 bytes: three loads from one stretch of memory)
                    cur = r; srcA = K.rows[3 * r]; srcB = K.rows[3 * r + 1];
                    const uint64_t lk = (uint64_t)K.rows[3 * r + 2];
                    len = (int)(uint32_t)lk; ka = (int)(uint32_t)(lk >> 32);
                }
                const int64_t j = c - (K.pad_side ? W - len : 0);     // the index inside the content
                const bool in = j >= 0 && j < len;
                const int64_t seam = (int64_t)fb + ka, second = seam + ns;      // the first separator, the first id of B
                int32_t v = K.pad_id;
                if (in) {
                    if (fb && j == 0) v = K.bos_id;
                    else if (fe && j == len - 1) v = K.eos_id;
                    else if (j >= seam && j < second) v = K.sep_id;
                    else {
                        const int64_t s = j < seam ? srcA + j - fb : srcB + j - second;
                        if (s >= 0 && s < K.ids_cap) v = tkz_load_nt(K.ids + s);
                    }
                }
                tkz_store_nt(K.out + q, v);
                if (K.mask) tkz_store_nt(K.mask + q, (uint8_t)(in ? 1 : 0));
                if (K.type_ids) tkz_store_nt(K.type_ids + q, (uint8_t)(in && j >= second ? 1 : 0));
                if (K.pos) tkz_store_nt(K.pos + q, in ? (int32_t)j : 0);
            }
            r += rstep; c += cstep;
            if (c >= W) { c -= W; ++r; }
        }
    }
}
// (the bracket: K_DOCOFFS's again, as launch_pad.  The width is known on the device only: the writing grid is sized for the positions the caller's buffer holds,
//  n_pairs * max_len at most -- beyond kPairGridMax workgroups both kernels stride)
void launch_pairs(const Launch& L, PairParams K) {
    const auto capped = [](int64_t g) { return g < 1 ? 1 : (g > kPairGridMax ? kPairGridMax : g); };
    const int64_t most = K.n_pairs > 0 && K.out_cap / K.max_len >= K.n_pairs ? K.n_pairs * K.max_len : K.out_cap;
    K.nparts = (int32_t)capped(cdiv(K.n_pairs, kThreads));
    TKZ_LAUNCH(k_pair_lens, K.nparts, kThreads, L.stream, K);
    TKZ_LAUNCH(k_pair_write, capped(cdiv(cdiv(most, kPairTile), kThreads / 64)), kThreads, L.stream, K);
    hook(L, K_DOCOFFS, 1);
}

// -------------------------------------------------------------------------------------------------
// Token-budget buckets (tkz_encode_batch_budgeted_device; tkz.h states the rule), behind the bucketed call's sequence up to the sort's last k_bkt_scatter, which
// is reused unchanged (order, rank, and slen / ssrc in sorted order): the sorted rows cut greedily into buckets of at most bucket_rows rows and at most
// token_budget positions (rows * width), every bucket padded to ITS OWN longest row.  Where a bucket ends depends on where the one before it ended; the chain
// that follows from that is walked over the RUNS of equal width -- 65 at L = 512, M = 8 -- and never over the buckets.
//   k_tbk_mark   a lane a sorted row: a row whose width differs from the row before it starts a run.  Pass 0 counts the marks of every group of 64 rows (one
//                ballot) and clears the runs' bucket counts; behind the scan of the counts pass 1 stores (first row, width) of every run at its ordinal.
//   k_tbk_chain  ONE wavefront, the only sequential stage.  It carries the entry row -- the first row no bucket holds yet -- from run to run.  Inside a run all
//                buckets have R_w = min(B, T / w) rows (B for w == 0), so their starts are an arithmetic progression and the run needs four numbers, not a
//                step a bucket.  Ascending, the bucket that crosses the run's end takes its width from its LAST row: it reaches into run m while
//                first[m] - start < R_w(m), which only gets harder with m -- the 64 lanes test 64 following runs with one ballot, so a bucket that swallows
//                whole runs costs a step, not one a run.  Descending, a bucket takes its width from its FIRST row and simply runs on over the run's end: the
//                next entry is the first start at or behind the end, and the lanes find the run it lies in (first[m] <= entry) the same way.  Runs jumped
//                over keep the zero pass 0 gave them.  The wavefront also adds up n_buckets and P.
//   k_tbk_table  behind the scan of the buckets a run: a lane a bucket finds its run by ONE search, then its first row, R_b, W_b and R_b * W_b.
//   (k_scan_partials64, k_scan_top, k_scan_final64: the 64-bit scan of R_b * W_b -> the bucket offsets.)
//   k_tbk_write  {total, P, n_cut} and n_buckets stored by one lane, both capacities held against them HERE, the bucket arrays copied to the caller; then
//                k_bkt_write's loop with a bucket's first row and row count read from the table: one search a tile, no division a position, the next
//                group's loads requested before this group's stores, every store tkz_store_nt.
// Nothing is added up in memory and nothing depends on timing: the same input gives the same bytes on every run.
// Known limit: with M = 1 and a very large L there are as many runs as distinct lengths, min(n_docs, L) at most, and the chain has that many steps.
// -------------------------------------------------------------------------------------------------
TKZ_KERNEL(256) void k_pad_lens(PadParams K);
TKZ_KERNEL(256) void k_bkt_hist(BktParams K, int shift, const uint32_t* keys, int64_t ntiles);
TKZ_KERNEL(256) void k_bkt_scatter(BktParams K, int shift, const uint32_t* keys, const int64_t* idx, uint32_t* keys_out, int64_t* idx_out, int64_t ntiles, int last);
static_assert(kTbkMarkTile == kThreads && kTbkLook == 64, "a lane a row, a lane a run");
// w(len): the width of a row of that length (tkz.h)
TKZ_DEV int64_t tkz_tbk_width(const PadParams& Q, int64_t len) {
    if (len <= 0) return 0;
    if (Q.pad_multiple == 0) return Q.max_len;
    const int64_t w = (len + Q.pad_multiple - 1) / Q.pad_multiple * Q.pad_multiple;
    return w < Q.max_len ? w : Q.max_len;
}
// R_w: the rows of a bucket all of whose rows have width w
TKZ_DEV int64_t tkz_tbk_rows(const TbkParams& K, int64_t w) {
    const int64_t B = K.bkt.bucket_rows, r = w > 0 ? K.token_budget / w : B;
    return r < B ? r : B;
}
TKZ_KERNEL(256) void k_tbk_mark(TbkParams K, int pass) {
    const PadParams& Q = K.bkt.pad;
    if (Q.counters[0] != 0) return;                            // (a failed attempt: slen means nothing)
    const int64_t r = simt::bid() * kTbkMarkTile + simt::tid(), n = Q.n_docs;
    int64_t w = 0;
    bool mark = false;
    if (r < n) { w = tkz_tbk_width(Q, K.bkt.slen[r]); mark = r == 0 || tkz_tbk_width(Q, K.bkt.slen[r - 1]) != w; }
    const uint64_t m = simt::ballot(mark);
    if (pass == 0) {
        if (simt::lane() == 0 && r < n) K.mark_cnt[r >> 6] = tkz_popc64(m);
        if (r < K.run_cap) K.run_nbk[r] = 0;                   // (run_cap <= n_docs: the grid covers it)
    } else if (mark) {
        const int64_t j = K.mark_base[r >> 6] + tkz_popc64(m & tkz_lowmask(simt::lane()));
        if (j >= 0 && j < K.run_cap) { K.run_first[j] = r; K.run_w[j] = (int32_t)w; }      // (always, by construction)
    }
}
// the runs from k on that pass a test which only gets harder with the run: 64 at a time, a ballot each; the return value is the first run that fails (or n_runs)
template <class Test> TKZ_DEV int64_t tkz_tbk_ahead(const TbkParams& K, int64_t k, int64_t nruns, Test passes) {
    for (;;) {
        const int64_t m = k + simt::lane();
        const bool ok = m < nruns && passes(K.run_first[m], (int64_t)K.run_w[m]);
        const int c = tkz_popc64(simt::ballot(ok));
        k += c;
        if (c < kTbkLook) return k;
    }
}
TKZ_KERNEL(256) void k_tbk_chain(TbkParams K) {
    const PadParams& Q = K.bkt.pad;
    if (Q.counters[0] != 0) return;
    const int64_t n = Q.n_docs;
    int64_t nruns = *K.n_runs;
    nruns = nruns < K.run_cap ? nruns : K.run_cap;
    int64_t s = 0, j = 0, nbk = 0, P = 0;                      // the entry row, its run, the buckets and the positions so far: the same in all 64 lanes
    while (s < n && j < nruns) {
        const int64_t end = j + 1 < nruns ? K.run_first[j + 1] : n, w = K.run_w[j], R = tkz_tbk_rows(K, w);
        int64_t nreg, cross = 0, nb, s2, j2;
        if (K.bkt.descending) {                                 // every bucket that STARTS in the run has the run's width and R rows (the batch's last: what is left)
            nreg = nb = (end - s + R - 1) / R;
            s2 = s + nb * R;
            P += ((s2 < n ? s2 : n) - s) * w;
            j2 = s2 < n ? tkz_tbk_ahead(K, j + 1, nruns, [&](int64_t first, int64_t) { return first <= s2; }) - 1 : nruns;
        } else {                                                // the buckets that END in the run, then the one that crosses its end
            nreg = nb = (end - s) / R;
            s2 = s + nreg * R; j2 = j + 1;
            P += nreg * R * w;
            if (s2 < end) {
                const int64_t k = tkz_tbk_ahead(K, j + 1, nruns, [&](int64_t first, int64_t wm) { return first - s2 < tkz_tbk_rows(K, wm); }) - 1;      // (the last run it reaches)
                const int64_t kend = k + 1 < nruns ? K.run_first[k + 1] : n, wk = K.run_w[k], most = s2 + tkz_tbk_rows(K, wk);
                cross = most < kend ? most : kend;
                P += (cross - s2) * wk;
                ++nb;
                j2 = cross < kend ? k : k + 1;
                s2 = cross;
            }
        }
        if (simt::lane() == 0) { K.run_entry[j] = s; K.run_r[j] = R; K.run_nreg[j] = nreg; K.run_cross[j] = cross; K.run_nbk[j] = (int32_t)nb; }
        nbk += nb; s = s2; j = j2;
    }
    if (simt::lane() == 0) { K.fig[0] = nbk; K.fig[1] = P; }
}
TKZ_KERNEL(256) void k_tbk_table(TbkParams K) {
    const PadParams& Q = K.bkt.pad;
    const int64_t b = simt::bid() * simt::nthreads() + simt::tid(), n = Q.n_docs;
    if (b >= K.tbl_cap || Q.counters[0] != 0) return;
    const int64_t nbk = K.fig[0];
    int64_t cnt = 0;
    if (b < nbk && nbk <= K.bucket_cap) {
        int64_t nruns = *K.n_runs;
        nruns = nruns < K.run_cap ? nruns : K.run_cap;
        const int64_t j = tkz_last_le(K.run_bbase, 0, nruns - 1, b);      // (runs without buckets repeat their neighbour's base: the last of them has the bucket)
        const int64_t i = b - K.run_bbase[j], R = K.run_r[j], r0 = K.run_entry[j] + i * R;
        int64_t r1 = r0 + R < n ? r0 + R : n, W = K.run_w[j];
        if (i >= K.run_nreg[j]) { r1 = K.run_cross[j]; W = r1 > r0 && r1 <= n ? tkz_tbk_width(Q, K.bkt.slen[r1 - 1]) : 0; }      // (the crossing bucket: its LAST row's width)
        K.brow[b] = r0; K.bw[b] = (int32_t)W;
        if (b == nbk - 1) K.brow[nbk] = n;
        cnt = (r1 - r0) * W;
    }
    K.bkt.bkt_cnt[b] = cnt;
}
// a lane's place in the rows: bucket b (its first sorted row r0, its width W), row i and column c of it, and the positions from here to the bucket's end
struct TbkCursor { int64_t b, r0, left; uint32_t W, i, c, rstep, cstep; };
TKZ_DEV void tkz_tbk_enter(const TbkParams& K, TbkCursor& s) {      // the first row, W, the steps of 64 positions and the bucket's positions for bucket s.b
    s.r0 = K.brow[s.b];
    s.W = (uint32_t)K.bw[s.b];
    s.left = (K.brow[s.b + 1] - s.r0) * (int64_t)s.W;
    s.i = 0; s.c = 0;
    s.rstep = s.W && s.W < 64u ? 64u / s.W : 0u; s.cstep = s.W && s.W < 64u ? 64u % s.W : 64u;
}
TKZ_DEV void tkz_tbk_step(const TbkParams& K, TbkCursor& s, uint32_t delta, int64_t nbk) {      // delta <= 64 positions on; the position stays below P
    while ((int64_t)delta >= s.left) {
        if (s.b + 1 >= nbk) { s.left = INT64_MAX; return; }      // (never below P)
        delta -= (uint32_t)s.left;
        ++s.b;
        tkz_tbk_enter(K, s);
    }
    s.left -= delta;
    if (s.W >= 64u) { s.c += delta; if (s.c >= s.W) { s.c -= s.W; ++s.i; } }
    else if (delta == 64u) { s.i += s.rstep; s.c += s.cstep; if (s.c >= s.W) { s.c -= s.W; ++s.i; } }
    else { const uint32_t x = s.c + delta; s.i += x / s.W; s.c = x % s.W; }
}
TKZ_KERNEL(256) void k_tbk_write(TbkParams K) {
    const PadParams& Q = K.bkt.pad;
    if (Q.counters[0] != 0) return;
    const int lane = simt::lane();
    const int64_t nwaves = simt::nblocks() * (kThreads / 64), wave0 = simt::bid() * (kThreads / 64) + simt::wave();
    const int64_t nbk = K.fig[0], P = K.fig[1], n = Q.n_docs;
    if (wave0 == 0) {                                           // the cut documents, from k_pad_lens' partials
        int64_t n_cut = 0;
        for (int i = lane; i < Q.nparts; i += 64) n_cut += Q.part_cut[i];
        for (int m = 32; m >= 1; m >>= 1) n_cut += tkz_shfl64(n_cut, lane ^ m);
        if (lane == 0) { Q.totals[0] = *Q.grand; Q.totals[1] = P; Q.totals[2] = n_cut; *K.n_buckets_out = nbk; }
    }
    if (nbk > K.bucket_cap) return;                             // (the bucket arrays do not fit: the figures are all that is written)
    for (int64_t b = simt::bid() * simt::nthreads() + simt::tid(); b <= nbk; b += simt::nblocks() * simt::nthreads()) {
        K.bkt.bucket_offs[b] = K.bkt.boffs[b]; K.bucket_rows_out[b] = K.brow[b];
        if (b < nbk) K.bkt.widths[b] = K.bw[b];
    }
    if (P <= 0 || P > Q.out_cap) return;                        // (nothing to write; or the rows do not fit)
    const int64_t ntile = (P + kBktTile - 1) / kBktTile;
    const int fb = Q.bos_id >= 0 ? 1 : 0, fe = Q.eos_id >= 0 ? 1 : 0;
    for (int64_t t = wave0; t < ntile; t += nwaves) {
        const int64_t q0 = t * kBktTile, q1 = q0 + kBktTile < P ? q0 + kBktTile : P;
        TbkCursor s;
        s.b = tkz_last_le(K.bkt.boffs, 0, nbk - 1, q0);         // (wave-uniform: one search a tile; offsets that repeat -- buckets of width 0 -- give the last)
        tkz_tbk_enter(K, s);
        {   // the tile's first position: one 64-bit division a tile, then the lane's own by a step
            const int64_t rel = q0 - K.bkt.boffs[s.b], row = s.W ? rel / (int64_t)s.W : 0;
            s.i = (uint32_t)row; s.c = (uint32_t)(rel - row * (int64_t)s.W); s.left -= rel;
        }
        int64_t cur = -1, src = 0;
        int len = 0;
        // what a lane stores at its position: the index inside the content (or -1: padding) and the id
        bool live = q0 + lane < q1;
        int32_t j = -1, v = Q.pad_id;
        for (int64_t g = q0 - 64; g < q1; g += 64) {
            // the NEXT group's values first: its loads are in flight while this group's are stored
            const bool live2 = g + 64 + lane < q1;
            int32_t j2 = -1, v2 = Q.pad_id;
            if (live2) {
                tkz_tbk_step(K, s, g < q0 ? (uint32_t)lane : 64u, nbk);
                const int64_t r = s.r0 + s.i;
                if (r != cur) { cur = r; len = r < n ? K.bkt.slen[r] : 0; src = r < n ? K.bkt.ssrc[r] : 0; }
                const int64_t jj = (int64_t)s.c - (Q.pad_side ? (int64_t)s.W - len : 0);     // the index inside the content
                if (jj >= 0 && jj < len) {
                    j2 = (int32_t)jj;
                    const int64_t a = src + jj - fb;
                    if (fb && jj == 0) v2 = Q.bos_id;
                    else if (fe && jj == len - 1) v2 = Q.eos_id;
                    else if (a >= 0 && a < Q.ids_cap) v2 = tkz_load_nt(Q.ids + a);
                }
            }
            if (g >= q0 && live) {
                const int64_t q = g + lane;
                tkz_store_nt(Q.out + q, v);
                if (Q.mask) tkz_store_nt(Q.mask + q, (uint8_t)(j >= 0 ? 1 : 0));
                if (Q.pos) tkz_store_nt(Q.pos + q, j >= 0 ? j : 0);
            }
            live = live2; j = j2; v = v2;
        }
    }
}
int64_t tbk_run_cap(int64_t n_docs, int64_t max_len, int64_t pad_multiple) {
    const int64_t widths = pad_multiple == 0 ? 2 : cdiv(max_len, pad_multiple) + 1;      // (0, the multiples of M below L, L)
    return n_docs < widths ? (n_docs < 1 ? 1 : n_docs) : widths;
}
int64_t tbk_mark_groups(int64_t n_docs) { return grid1(cdiv(n_docs, 64)); }
// (the bracket: K_DOCOFFS's again, as launch_bucketed.  n_buckets and P are known on the device only: the table's grid and scan are sized for min(n_docs,
//  bucket_cap) buckets, the writing grid for the positions the caller's buffer holds, the run scan for the runs a batch of this L and M can have)
void launch_budgeted(const Launch& L, TbkParams K) {
    const auto capped = [](int64_t g) { return g < 1 ? 1 : (g > kPadGridMax ? kPadGridMax : g); };
    BktParams& S = K.bkt;
    const int64_t n = S.pad.n_docs, ntiles = bkt_sort_tiles(n);
    const int64_t most = n > 0 && S.pad.out_cap / S.pad.max_len >= n ? n * S.pad.max_len : S.pad.out_cap;
    S.pad.nparts = (int32_t)capped(cdiv(n, kThreads));
    S.npass = bkt_passes(S.pad.max_len);
    TKZ_LAUNCH(k_pad_lens, S.pad.nparts, kThreads, L.stream, S.pad);
    for (int p = 0; p < S.npass; ++p) {                         // (launch_bucketed's sort, as it is)
        const bool last = p + 1 == S.npass;
        const uint32_t* keys = p == 0 ? nullptr : (p & 1 ? S.key_a : S.key_b);
        const int64_t* idx = p == 0 ? nullptr : (p & 1 ? S.idx_a : S.idx_b);
        TKZ_LAUNCH(k_bkt_hist, ntiles, kThreads, L.stream, S, 8 * p, keys, ntiles);
        launch_scan2(L, 256 * ntiles, S.scan_bsum, S.hist, S.hist_base, S.hist_total, 1, nullptr, nullptr, nullptr, 1, -1);
        TKZ_LAUNCH(k_bkt_scatter, ntiles, kThreads, L.stream, S, 8 * p, keys, idx, last ? (uint32_t*)nullptr : (p & 1 ? S.key_b : S.key_a),
                   last ? S.order : (p & 1 ? S.idx_b : S.idx_a), ntiles, last ? 1 : 0);
    }
    const int64_t gmark = grid1(cdiv(n, kTbkMarkTile)), nblk = grid1(cdiv(K.tbl_cap, kScanBlock));
    TKZ_LAUNCH(k_tbk_mark, gmark, kThreads, L.stream, K, 0);
    launch_scan2(L, tbk_mark_groups(n), S.scan_bsum, K.mark_cnt, K.mark_base, K.n_runs, 1, nullptr, nullptr, nullptr, 1, -1);
    TKZ_LAUNCH(k_tbk_mark, gmark, kThreads, L.stream, K, 1);
    TKZ_LAUNCH(k_tbk_chain, 1, 64, L.stream, K);
    launch_scan2(L, K.run_cap, S.scan_bsum, K.run_nbk, K.run_bbase, K.fig + 2, 1, nullptr, nullptr, nullptr, 1, -1);
    TKZ_LAUNCH(k_tbk_table, grid1(cdiv(K.tbl_cap, kThreads)), kThreads, L.stream, K);
    TKZ_LAUNCH(k_scan_partials64, nblk, kThreads, L.stream, (const int64_t*)S.bkt_cnt, K.tbl_cap, S.scan_bsum);
    TKZ_LAUNCH(k_scan_top, 1, kThreads, L.stream, S.scan_bsum, nblk, S.boffs + K.tbl_cap);
    TKZ_LAUNCH(k_scan_final64, nblk, kThreads, L.stream, (const int64_t*)S.bkt_cnt, K.tbl_cap, (const int64_t*)S.scan_bsum, S.boffs);
    TKZ_LAUNCH(k_tbk_write, capped(cdiv(cdiv(most, kBktTile), kThreads / 64)), kThreads, L.stream, K);
    hook(L, K_DOCOFFS, 1);
}

// -------------------------------------------------------------------------------------------------
// Length-bucketed padded rows (tkz_encode_batch_bucketed_device; tkz.h states the rule), behind the padded call's sequence up to k_pad_lens, which is reused
// unchanged (lens, src, the cut documents of every workgroup): the documents sorted by len, cut into buckets of bucket_rows sorted rows, every bucket padded to
// ITS OWN longest row.
//   k_bkt_hist     a pass of the stable LSD radix sort, 8 bits a pass: a workgroup per tile of kBktSortTile keys, the tile's count of every digit, digit-major.
//   k_bkt_scatter  the same tile again behind the scan of the counts: key and document to base[digit][tile] + the key's rank among the tile's EARLIER keys of
//                  its digit; the LAST pass stores the documents into `order`, the inverse into `rank`, and lens / src of every document at its SORTED row (slen,
//                  ssrc: what the table and the writer read -- one dependent load less a row than through `order`).  Both kernels get that rank from tkz_bkt_rank: a wavefront owns four consecutive groups of 64 keys; inside a group the lanes
//                  of one digit find each other with eight ballots (a lane's rank: the lanes below it in that set), the set's lowest lane stores its size into
//                  s_cnt[group][digit]; after a barrier thread t turns column t into its exclusive prefix over the 16 groups -- the column's sum is the tile's
//                  count of digit t --, after another a lane adds s_cnt[its group][its digit].  Nothing is added up in memory and no order depends on timing:
//                  the sort gives the same permutation on every run.
//   k_bkt_table    a lane a bucket: the longest len is that of the bucket's last (ascending) or first (descending) sorted row -- no reduction --, W_b, R_b * W_b.
//   (k_scan_partials64, k_scan_top, k_scan_final64: the 64-bit scan of R_b * W_b -> the bucket offsets and P; R_b * W_b does not fit 32 bits.)
//   k_bkt_write    the bucket offsets copied to the caller, {total, P, n_cut} stored by one lane, P held against out_cap HERE; then k_pad_write's loop with the
//                  width looked up per bucket: a wavefront per tile of kBktTile output positions, grid-strided.  A tile finds its first bucket by ONE search
//                  over the offsets (wave-uniform) and its row and column there by one 64-bit division; a lane then carries (bucket, row, column, positions
//                  left in the bucket) forward by 64 positions with additions -- a 32-bit division only where it ENTERS a bucket narrower than 64 columns --
//                  so a tile may span a hundred buckets and a row three tiles.  The next group's slen / ssrc and id are requested before this group's
//                  stores.  Every store of a row is tkz_store_nt, all 64 lanes, consecutive addresses.
// -------------------------------------------------------------------------------------------------
TKZ_KERNEL(256) void k_pad_lens(PadParams K);
constexpr int kBktGroups = kBktSortTile / 64, kBktPer = kBktSortTile / kThreads;
// the keys of a thread: key j of the tile's group wave * kBktPer + j, lane-th of it; pass 0 makes them from lens
TKZ_DEV void tkz_bkt_keys(const BktParams& K, const uint32_t* keys, int shift, int64_t* at, uint32_t* key, uint32_t* dig, bool* ok) {
    const int64_t i0 = simt::bid() * kBktSortTile + simt::wave() * (kBktPer * 64) + simt::lane();
#pragma unroll
    for (int j = 0; j < kBktPer; ++j) {
        const int64_t i = i0 + j * 64;
        at[j] = i; ok[j] = i < K.pad.n_docs;
        uint32_t k = 0;
        if (ok[j]) k = keys ? keys[i] : (K.descending ? (uint32_t)(K.pad.max_len - K.pad.lens[i]) : (uint32_t)K.pad.lens[i]);
        key[j] = k; dig[j] = (k >> shift) & 255u;
    }
}
// rnk[j]: the number of the tile's keys IN FRONT of key j with its digit; the return value: the tile's keys with digit tid()
TKZ_DEV int tkz_bkt_rank(int (*s_cnt)[256], const uint32_t* dig, const bool* ok, int* rnk) {
    const int tid = simt::tid(), g0 = simt::wave() * kBktPer;
    const uint64_t below = tkz_lowmask(simt::lane());
    for (int g = 0; g < kBktGroups; ++g) s_cnt[g][tid] = 0;
    simt::sync();
#pragma unroll
    for (int j = 0; j < kBktPer; ++j) {
        uint64_t m = simt::ballot(ok[j]);
#pragma unroll
        for (int b = 0; b < 8; ++b) { const bool bit = (dig[j] >> b) & 1u; const uint64_t has = simt::ballot(bit); m &= bit ? has : ~has; }
        rnk[j] = tkz_popc64(m & below);
        if (ok[j] && rnk[j] == 0) s_cnt[g0 + j][dig[j]] = tkz_popc64(m);
    }
    simt::sync();
    int run = 0;
    for (int g = 0; g < kBktGroups; ++g) { const int c = s_cnt[g][tid]; s_cnt[g][tid] = run; run += c; }
    simt::sync();
#pragma unroll
    for (int j = 0; j < kBktPer; ++j) if (ok[j]) rnk[j] += s_cnt[g0 + j][dig[j]];
    return run;
}
TKZ_KERNEL(256) void k_bkt_hist(BktParams K, int shift, const uint32_t* keys, int64_t ntiles) {
    TKZ_SHARED int s_cnt[kBktGroups][256];
    if (K.pad.counters[0] != 0) return;                        // (a failed attempt: lens means nothing)
    int64_t at[kBktPer]; uint32_t key[kBktPer], dig[kBktPer]; bool ok[kBktPer]; int rnk[kBktPer];
    tkz_bkt_keys(K, keys, shift, at, key, dig, ok);
    K.hist[(int64_t)simt::tid() * ntiles + simt::bid()] = tkz_bkt_rank(s_cnt, dig, ok, rnk);
}
TKZ_KERNEL(256) void k_bkt_scatter(BktParams K, int shift, const uint32_t* keys, const int64_t* idx, uint32_t* keys_out, int64_t* idx_out, int64_t ntiles, int last) {
    TKZ_SHARED int s_cnt[kBktGroups][256];
    TKZ_SHARED int64_t s_base[256];
    if (K.pad.counters[0] != 0) return;
    int64_t at[kBktPer]; uint32_t key[kBktPer], dig[kBktPer]; bool ok[kBktPer]; int rnk[kBktPer];
    tkz_bkt_keys(K, keys, shift, at, key, dig, ok);
    s_base[simt::tid()] = K.hist_base[(int64_t)simt::tid() * ntiles + simt::bid()];
    (void)tkz_bkt_rank(s_cnt, dig, ok, rnk);                   // (its barriers order s_base as well)
    const int64_t n = K.pad.n_docs;
#pragma unroll
    for (int j = 0; j < kBktPer; ++j) {
        if (!ok[j]) continue;
        const int64_t to = s_base[dig[j]] + rnk[j], d = idx ? idx[at[j]] : at[j];
        if (to < 0 || to >= n || d < 0 || d >= n) continue;      // (never, by construction: nothing is stored outside the arrays whatever the counts say)
        if (keys_out) keys_out[to] = key[j];
        idx_out[to] = d;
        if (last) { K.slen[to] = K.pad.lens[d]; K.ssrc[to] = K.pad.src[d]; if (K.rank) K.rank[d] = to; }      // (the rows' lens and src in SORTED order: the writer's)
    }
}
TKZ_KERNEL(256) void k_bkt_table(BktParams K) {
    const PadParams& Q = K.pad;
    const int64_t b = simt::bid() * simt::nthreads() + simt::tid(), n = Q.n_docs;
    if (b >= K.n_buckets) return;
    int64_t cnt = 0;
    if (Q.counters[0] == 0) {
        const int64_t r0 = b * K.bucket_rows, r1 = r0 + K.bucket_rows < n ? r0 + K.bucket_rows : n;
        const int64_t longest = K.slen[K.descending ? r0 : r1 - 1], L = Q.max_len, M = Q.pad_multiple;
        int64_t W = 0;
        if (longest > 0) { W = M == 0 ? L : (longest + M - 1) / M * M; W = W < L ? W : L; }
        K.widths[b] = (int32_t)W;
        cnt = (r1 - r0) * W;
    }
    K.bkt_cnt[b] = cnt;
}
// a lane's place in the rows: bucket b (its first sorted row r0, its width W), row i and column c of it, and the positions from here to the bucket's end
struct BktCursor { int64_t b, r0, left; uint32_t W, i, c, rstep, cstep; };
TKZ_DEV void tkz_bkt_enter(const BktParams& K, BktCursor& s) {      // W, the steps of 64 positions and the bucket's positions for bucket s.b
    const int64_t rows = s.r0 + K.bucket_rows < K.pad.n_docs ? K.bucket_rows : K.pad.n_docs - s.r0;
    s.W = (uint32_t)K.widths[s.b];
    s.left = rows * (int64_t)s.W;
    s.i = 0; s.c = 0;
    s.rstep = s.W && s.W < 64u ? 64u / s.W : 0u; s.cstep = s.W && s.W < 64u ? 64u % s.W : 64u;
}
TKZ_DEV void tkz_bkt_step(const BktParams& K, BktCursor& s, uint32_t delta) {      // delta <= 64 positions on; the position stays below P
    while ((int64_t)delta >= s.left) {
        if (s.b + 1 >= K.n_buckets) { s.left = INT64_MAX; return; }      // (never below P)
        delta -= (uint32_t)s.left;
        ++s.b; s.r0 += K.bucket_rows;
        tkz_bkt_enter(K, s);
    }
    s.left -= delta;
    if (s.W >= 64u) { s.c += delta; if (s.c >= s.W) { s.c -= s.W; ++s.i; } }
    else if (delta == 64u) { s.i += s.rstep; s.c += s.cstep; if (s.c >= s.W) { s.c -= s.W; ++s.i; } }
    else { const uint32_t x = s.c + delta; s.i += x / s.W; s.c = x % s.W; }
}
TKZ_KERNEL(256) void k_bkt_write(BktParams K) {
    const PadParams& Q = K.pad;
    if (Q.counters[0] != 0) return;
    const int lane = simt::lane();
    const int64_t nwaves = simt::nblocks() * (kThreads / 64), wave0 = simt::bid() * (kThreads / 64) + simt::wave();
    const int64_t nb = K.n_buckets, n = Q.n_docs;
    for (int64_t b = simt::bid() * simt::nthreads() + simt::tid(); b <= nb; b += simt::nblocks() * simt::nthreads()) K.bucket_offs[b] = K.boffs[b];
    const int64_t P = K.boffs[nb];
    if (wave0 == 0) {                                           // the cut documents, from k_pad_lens' partials
        int64_t n_cut = 0;
        for (int i = lane; i < Q.nparts; i += 64) n_cut += Q.part_cut[i];
        for (int m = 32; m >= 1; m >>= 1) n_cut += tkz_shfl64(n_cut, lane ^ m);
        if (lane == 0) { Q.totals[0] = *Q.grand; Q.totals[1] = P; Q.totals[2] = n_cut; }
    }
    if (P <= 0 || P > Q.out_cap) return;                        // (nothing to write; or the rows do not fit: the totals are all that is written)
    const int64_t ntile = (P + kBktTile - 1) / kBktTile;
    const int fb = Q.bos_id >= 0 ? 1 : 0, fe = Q.eos_id >= 0 ? 1 : 0;
    for (int64_t t = wave0; t < ntile; t += nwaves) {
        const int64_t q0 = t * kBktTile, q1 = q0 + kBktTile < P ? q0 + kBktTile : P;
        BktCursor s;
        s.b = tkz_last_le(K.boffs, 0, nb - 1, q0);             // (wave-uniform: one search a tile; offsets that repeat -- buckets of width 0 -- give the last)
        s.r0 = s.b * K.bucket_rows;
        tkz_bkt_enter(K, s);
        {   // the tile's first position: one 64-bit division a tile, then the lane's own by a step
            const int64_t rel = q0 - K.boffs[s.b], row = s.W ? rel / (int64_t)s.W : 0;
            s.i = (uint32_t)row; s.c = (uint32_t)(rel - row * (int64_t)s.W); s.left -= rel;
        }
        int64_t cur = -1, src = 0;
        int len = 0;
        // what a lane stores at its position: the index inside the content (or -1: padding) and the id
        bool live = q0 + lane < q1;
        int32_t j = -1, v = Q.pad_id;
        for (int64_t g = q0 - 64; g < q1; g += 64) {
            // the NEXT group's values first: its loads are in flight while this group's are stored
            const bool live2 = g + 64 + lane < q1;
            int32_t j2 = -1, v2 = Q.pad_id;
            if (live2) {
                tkz_bkt_step(K, s, g < q0 ? (uint32_t)lane : 64u);
                const int64_t r = s.r0 + s.i;
                if (r != cur) { cur = r; len = r < n ? K.slen[r] : 0; src = r < n ? K.ssrc[r] : 0; }
                const int64_t jj = (int64_t)s.c - (Q.pad_side ? (int64_t)s.W - len : 0);     // the index inside the content
                if (jj >= 0 && jj < len) {
                    j2 = (int32_t)jj;
                    const int64_t a = src + jj - fb;
                    if (fb && jj == 0) v2 = Q.bos_id;
                    else if (fe && jj == len - 1) v2 = Q.eos_id;
                    else if (a >= 0 && a < Q.ids_cap) v2 = tkz_load_nt(Q.ids + a);
                }
            }
            if (g >= q0 && live) {
                const int64_t q = g + lane;
                tkz_store_nt(Q.out + q, v);
                if (Q.mask) tkz_store_nt(Q.mask + q, (uint8_t)(j >= 0 ? 1 : 0));
                if (Q.pos) tkz_store_nt(Q.pos + q, j >= 0 ? j : 0);
            }
            live = live2; j = j2; v = v2;
        }
    }
}
int bkt_passes(int64_t max_len) { int bits = 1; while (bits < 32 && (max_len >> bits) != 0) ++bits; return (bits + 7) / 8; }
int64_t bkt_sort_tiles(int64_t n_docs) { return grid1(cdiv(n_docs, kBktSortTile)); }
// (the bracket: K_DOCOFFS's again, as launch_pad.  P is known on the device only: the writing grid is sized for the positions the caller's buffer holds,
//  n_docs * max_len at most -- beyond kPadGridMax workgroups k_pad_lens and k_bkt_write stride; the sort and the table have a workgroup a tile / 256 buckets)
void launch_bucketed(const Launch& L, BktParams K) {
    const auto capped = [](int64_t g) { return g < 1 ? 1 : (g > kPadGridMax ? kPadGridMax : g); };
    const int64_t n = K.pad.n_docs, ntiles = bkt_sort_tiles(n);
    const int64_t most = n > 0 && K.pad.out_cap / K.pad.max_len >= n ? n * K.pad.max_len : K.pad.out_cap;
    K.pad.nparts = (int32_t)capped(cdiv(n, kThreads));
    K.npass = bkt_passes(K.pad.max_len);
    TKZ_LAUNCH(k_pad_lens, K.pad.nparts, kThreads, L.stream, K.pad);
    for (int p = 0; p < K.npass; ++p) {
        const bool last = p + 1 == K.npass;
        const uint32_t* keys = p == 0 ? nullptr : (p & 1 ? K.key_a : K.key_b);
        const int64_t* idx = p == 0 ? nullptr : (p & 1 ? K.idx_a : K.idx_b);
        TKZ_LAUNCH(k_bkt_hist, ntiles, kThreads, L.stream, K, 8 * p, keys, ntiles);
        launch_scan2(L, 256 * ntiles, K.scan_bsum, K.hist, K.hist_base, K.hist_total, 1, nullptr, nullptr, nullptr, 1, -1);
        TKZ_LAUNCH(k_bkt_scatter, ntiles, kThreads, L.stream, K, 8 * p, keys, idx, last ? (uint32_t*)nullptr : (p & 1 ? K.key_b : K.key_a),
                   last ? K.order : (p & 1 ? K.idx_b : K.idx_a), ntiles, last ? 1 : 0);
    }
    const int64_t nblk = grid1(cdiv(K.n_buckets, kScanBlock));
    TKZ_LAUNCH(k_bkt_table, grid1(cdiv(K.n_buckets, kThreads)), kThreads, L.stream, K);
    TKZ_LAUNCH(k_scan_partials64, nblk, kThreads, L.stream, (const int64_t*)K.bkt_cnt, K.n_buckets, K.scan_bsum);
    TKZ_LAUNCH(k_scan_top, 1, kThreads, L.stream, K.scan_bsum, nblk, K.boffs + K.n_buckets);
    TKZ_LAUNCH(k_scan_final64, nblk, kThreads, L.stream, (const int64_t*)K.bkt_cnt, K.n_buckets, (const int64_t*)K.scan_bsum, K.boffs);
    TKZ_LAUNCH(k_bkt_write, capped(cdiv(cdiv(most, kBktTile), kThreads / 64)), kThreads, L.stream, K);
    hook(L, K_DOCOFFS, 1);
}

// -------------------------------------------------------------------------------------------------
// Padded rows (tkz_encode_batch_padded_device; tkz.h states the rule), behind the plain document-granular launch sequence: a row a document, cut to max_len,
// framed, padded to the common width W on either side, with the mask and the position inside the content.  The uncut ids and offsets O stay in the workspace.
//   k_pad_lens    a lane a document: n = O[d + 1] - O[d], k = min(n, L - f), lens[d] = k + f, src[d] = the index of the first kept id (O[d], or O[d + 1] - k
//                 for a cut at the front), out_offs[d] = O[d].  The largest len and the number of cut documents of a workgroup go into ONE partial each: the
//                 wavefronts' by shuffles, the four of them through 48 bytes of LDS.  Nothing is added up in memory, so the result is the same on every run.
//   k_pad_write   every wavefront reduces the partials (nparts <= kPadGridMax, from L2) to W and n_cut, one lane stores {total, W, n_cut}, and the kernel holds
//                 n_docs * W against out_cap itself: the host never waits for the width between the two launches.  The rows are dealt out by OUTPUT position,
//                 a wavefront per tile of kPadTile positions, grid-strided.  Row and column of a tile's first position cost one 64-bit division a TILE
//                 (wave-uniform); a lane steps them by 64 positions with additions and one conditional subtraction.  A row may be shorter than 64 columns (a
//                 group of 64 positions then spans many rows: the step is 64 / W rows and 64 % W columns) or longer than a tile.  A lane loads lens and src of
//                 its row only when its row changes.  It reads lens and src, not O: whoever fills the two arrays decides what is kept.
// Every store of a row is tkz_store_nt, all 64 lanes, consecutive addresses.
// -------------------------------------------------------------------------------------------------
TKZ_DEV int tkz_pad_wave_max(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const int o = simt::shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}
TKZ_DEV int64_t tkz_pad_wave_sum(int64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)simt::shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)simt::shfl_xor((int)(uint32_t)((uint64_t)v >> 32), m);
        v += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    return v;
}
TKZ_KERNEL(256) void k_pad_lens(PadParams K) {
    TKZ_SHARED int s_len[kThreads / 64];
    TKZ_SHARED int64_t s_cut[kThreads / 64];
    const bool bad = K.counters[0] != 0;                       // (a failed attempt: the offsets mean nothing, the caller's buffers are left alone)
    const int64_t f = (K.bos_id >= 0 ? 1 : 0) + (K.eos_id >= 0 ? 1 : 0), room = K.max_len - f;
    const int64_t stride = simt::nblocks() * simt::nthreads();
    int longest = 0;
    int64_t ncut = 0;
    if (!bad) for (int64_t d = simt::bid() * simt::nthreads() + simt::tid(); d < K.n_docs; d += stride) {
        const int64_t lo = K.offs[d], hi = K.offs[d + 1], n = hi - lo, k = n < room ? n : room;
        const int len = (int)(k + f);
        K.lens[d] = len;
        K.src[d] = K.cut_side ? hi - k : lo;
        if (K.out_offs) { K.out_offs[d] = lo; if (d == K.n_docs - 1) K.out_offs[K.n_docs] = hi; }
        longest = len > longest ? len : longest;
        ncut += n > room ? 1 : 0;
    }
    longest = tkz_pad_wave_max(longest);
    ncut = tkz_pad_wave_sum(ncut);
    if (simt::lane() == 0) { s_len[simt::wave()] = longest; s_cut[simt::wave()] = ncut; }
    simt::sync();
    if (simt::tid() == 0) {
        int64_t c = 0;
        for (int w = 0; w < simt::nthreads() / 64; ++w) { longest = s_len[w] > longest ? s_len[w] : longest; c += s_cut[w]; }
        K.part_len[simt::bid()] = longest;
        K.part_cut[simt::bid()] = c;
    }
}
TKZ_KERNEL(256) void k_pad_write(PadParams K) {
    if (K.counters[0] != 0) return;
    const int lane = simt::lane();
    const int64_t nwaves = simt::nblocks() * (kThreads / 64), wave0 = simt::bid() * (kThreads / 64) + simt::wave();
    // the width and the cut documents, from the partials
    int longest = 0;
    int64_t n_cut = 0;
    for (int i = lane; i < K.nparts; i += 64) {
        const int l = K.part_len[i];
        longest = l > longest ? l : longest;
        n_cut += K.part_cut[i];
    }
    longest = tkz_pad_wave_max(longest);
    n_cut = tkz_pad_wave_sum(n_cut);
    const int64_t L = K.max_len, M = K.pad_multiple;
    int64_t W = 0;
    if (longest > 0) { W = M == 0 ? L : (longest + M - 1) / M * M; W = W < L ? W : L; }
    W = (int64_t)simt::uniform64((uint64_t)W);
    if (wave0 == 0 && lane == 0) { K.totals[0] = *K.grand; K.totals[1] = W; K.totals[2] = n_cut; }
    if (W == 0 || K.n_docs > K.out_cap / W) return;            // (nothing to write; or the rows do not fit: the totals are all that is written)
    const int64_t N = K.n_docs * W, ntile = (N + kPadTile - 1) / kPadTile;
    const int fb = K.bos_id >= 0 ? 1 : 0, fe = K.eos_id >= 0 ? 1 : 0;
    // 64 positions on: rstep rows and cstep < W columns
    const int64_t rstep = W > 64 ? 0 : (int64_t)(64u / (uint32_t)W), cstep = W > 64 ? 64 : (int64_t)(64u % (uint32_t)W);
    for (int64_t t = wave0; t < ntile; t += nwaves) {
        const int64_t q0 = t * kPadTile, q1 = q0 + kPadTile < N ? q0 + kPadTile : N;
        const int64_t row0 = q0 / W, col0 = q0 - row0 * W;     // (wave-uniform: one division a tile)
        int64_t r, c;
        if (W >= 64) { r = row0; c = col0 + lane; if (c >= W) { c -= W; ++r; } }
        else { const uint32_t x = (uint32_t)col0 + (uint32_t)lane; r = row0 + (int64_t)(x / (uint32_t)W); c = (int64_t)(x % (uint32_t)W); }
        int64_t cur = -1, src = 0;
        int len = 0;
        for (int64_t g = q0; g < q1; g += 64) {
            const int64_t q = g + lane;
            if (q < q1) {
                if (r != cur) { cur = r; len = K.lens[r]; src = K.src[r]; }
                const int64_t j = c - (K.pad_side ? W - len : 0);     // the index inside the content
                const bool in = j >= 0 && j < len;
                int32_t v = K.pad_id;
                if (in) {
                    const int64_t s = src + j - fb;
                    if (fb && j == 0) v = K.bos_id;
                    else if (fe && j == len - 1) v = K.eos_id;
                    else if (s >= 0 && s < K.ids_cap) v = tkz_load_nt(K.ids + s);
                }
                tkz_store_nt(K.out + q, v);
                if (K.mask) tkz_store_nt(K.mask + q, (uint8_t)(in ? 1 : 0));
                if (K.pos) tkz_store_nt(K.pos + q, in ? (int32_t)j : 0);
            }
            r += rstep; c += cstep;
            if (c >= W) { c -= W; ++r; }
        }
    }
}
// (the bracket: K_DOCOFFS's again, as launch_pack.  The width is known on the device only: the writing grid is sized for the positions the caller's buffer
//  holds, n_docs * max_len at most -- beyond kPadGridMax workgroups both kernels stride)
void launch_pad(const Launch& L, PadParams K) {
    const auto capped = [](int64_t g) { return g < 1 ? 1 : (g > kPadGridMax ? kPadGridMax : g); };
    const int64_t most = K.n_docs > 0 && K.out_cap / K.max_len >= K.n_docs ? K.n_docs * K.max_len : K.out_cap;
    K.nparts = (int32_t)capped(cdiv(K.n_docs, kThreads));
    TKZ_LAUNCH(k_pad_lens, K.nparts, kThreads, L.stream, K);
    TKZ_LAUNCH(k_pad_write, capped(cdiv(cdiv(most, kPadTile), kThreads / 64)), kThreads, L.stream, K);
    hook(L, K_DOCOFFS, 1);
}

}  // namespace tkz
