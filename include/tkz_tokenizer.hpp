// tkz_tokenizer.hpp -- C++ host mirror of the reference's tokenizer interface (Encode, and Decode for a batch), over the
// C ABI of include/tkz.h.  Header-only; link with libtkz.so.
//
//   tkz::TikTokenizer          ITokenizer.Encode x2 + EncodeBatch     Tokenizer_C#/TokenizerLib/ITokenizer.cs:12,28
//                              EncodeBatchFlat: (ids, offsets) in page-locked buffers that are kept from call to call (tkz::FlatBatch)
//                              EncodeTrimSuffix / EncodeTrimPrefix x2   ITokenizer.cs:30-44, TikTokenizer.cs:288-579
//                              CountTokens / CountTokensBatch (+ Utf16): Encode(...).Count from the device's count entries, no ids
//                              EncodeWithOffsets / EncodeWithOffsetsBatch (+ Utf16): Encode, and where every token's text starts (bytes / code units)
//                              EncodeChunks / EncodeChunksBatch (+ Utf16): the text cut into chunks of at most maxTokenCount tokens, (ids, text) each
//                              EncodeChunksOverlap / EncodeChunksOverlapBatch (+ Utf16): the same with an overlap of at most `overlap` tokens between neighbours
//                              EncodeBatchPacked (std::string, std::u16string): the ids framed by bos / eos ids in rows of the context length, pos, seg_starts
//                              EncodeBatchPadded (std::string, std::u16string): a row a text, cut to maxLength, framed, padded to a common width; mask, pos, lens
//                              EncodeBatchBucketed (std::string, std::u16string): the same rows sorted by length, a width per bucket of bucketRows rows; order, rank
//                              EncodeBatchPairs (std::string, std::u16string): two texts a row, [bos] A sep B [eos], cut by a strategy, padded; mask, type ids, kept
//                              Decode / DecodeBatch (bytes), DecodeUtf16 / DecodeBatchUtf16 (the string's code units)   TikTokenizer.cs:586-604
//   tkz::TokenizerBuilder      CreateTokenizer(stream, specials, pattern)   TokenizerBuilder.cs:210-213
//
// Text is UTF-8 (std::string); the ...Utf16 methods take the code units of a .NET string (std::u16string) and hand them to the device's UTF-16 entries,
// special tokens and trimming included (tkz_encode_batch_special_utf16 / tkz_encode_batch_trim_utf16).  Special-token
// segmentation (EncodeInternal / FindNextSpecialToken, TikTokenizer.cs:141-170,230-241) runs on the host and
// every plain segment of a batch goes to the GPU in ONE tkz_encode_batch_utf8 call.  Errors are exceptions
// named after the reference's: FormatException -> tkz::FormatError, ArgumentException -> tkz::DuplicateRankError,
// KeyNotFoundException -> tkz::KeyNotFoundError, NotImplementedException -> tkz::NotImplementedError.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "tkz.h"

namespace tkz {

struct Error : std::runtime_error { int status; Error(int s, const std::string& m) : std::runtime_error(m), status(s) {} };
struct FormatError : Error { using Error::Error; };
struct DuplicateRankError : Error { using Error::Error; };
struct KeyNotFoundError : Error { using Error::Error; };
struct NotImplementedError : Error { using Error::Error; };

inline void check(tkz_status s) {
    if (s == TKZ_OK) return;
    const std::string m = tkz_last_error();
    switch (s) {
        case TKZ_E_FORMAT: throw FormatError(s, m);
        case TKZ_E_DUP_RANK: throw DuplicateRankError(s, m);
        case TKZ_E_KEY_NOT_FOUND: throw KeyNotFoundError(s, m);
        case TKZ_E_UNSUPPORTED: throw NotImplementedError(s, m);
        default: throw Error(s, m);
    }
}

using SpecialTokens = std::vector<std::pair<std::string, int32_t>>;   // registration order matters (alternation order)

// A grow-only page-locked host buffer (tkz_host_alloc): copies from and to it run at the PCIe rate.
class PinnedBuffer {
public:
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() { tkz_host_free(p_); }
    void* ensure(size_t bytes) {
        if (bytes > cap_) {
            tkz_host_free(p_); p_ = nullptr; cap_ = 0;
            const size_t want = bytes + bytes / 4 + 4096;
            check(tkz_host_alloc(want, &p_));
            cap_ = want;
        }
        return p_;
    }
    template <class T> T* as() const { return static_cast<T*>(p_); }
private:
    void* p_ = nullptr; size_t cap_ = 0;
};

// The result of TikTokenizer::EncodeBatchFlat: text t is ids()[offsets()[t] .. offsets()[t + 1]).  It owns the page-locked buffers the
// call works in (the gathered text, the ids, the offsets) and keeps them from call to call: hand the same FlatBatch to every call of a
// loop and nothing is allocated after the first.  The views are valid until the next call that is given this object.
class FlatBatch {
public:
    const int32_t* ids() const { return ids_; }
    const int64_t* offsets() const { return offsets_; }
    int64_t n_texts() const { return n_texts_; }
    int64_t n_ids() const { return n_texts_ >= 0 && offsets_ ? offsets_[n_texts_] : 0; }
    std::vector<int32_t> text(int64_t t) const { return std::vector<int32_t>(ids_ + offsets_[t], ids_ + offsets_[t + 1]); }
    // where the last call's time went, in milliseconds: the offsets pass, waiting for gathered sub-batches, inside tkz_encode_batch_utf8
    double last_offsets_ms = 0, last_wait_ms = 0, last_encode_ms = 0;
private:
    friend class TikTokenizer;
    PinnedBuffer in_bytes_, in_offs_, sub_offs_, out_ids_, out_offs_;
    std::vector<int32_t> spliced_ids_; std::vector<int64_t> spliced_offs_;     // (only when special tokens were spliced in on the host: the fallback)
    const int32_t* ids_ = nullptr; const int64_t* offsets_ = nullptr; int64_t n_texts_ = 0;
    double tokens_per_byte_ = 0;                                               // the densest batch seen: sizes the id buffer of the next one
};

class TikTokenizer {
public:
    TikTokenizer(const std::string& tikTokenBpeFile, SpecialTokens specialTokensEncoder, const std::string& pattern, int device = 0)
        : specials_(std::move(specialTokensEncoder)) {
        int32_t pat = 0;
        check(tkz_pattern_from_regex(pattern.c_str(), &pat));
        tkz_vocab* v = nullptr;
        check(tkz_vocab_from_tiktoken(reinterpret_cast<const uint8_t*>(tikTokenBpeFile.data()), tikTokenBpeFile.size(), &v));
        const tkz_status s = tkz_encoder_create(v, pat, device, &enc_);
        tkz_vocab_destroy(v);
        check(s);
        if (!specials_.empty()) {                              // the literals the device cuts out of the text (EncodeBatchFlat), in registration order
            std::vector<int32_t> ids; std::string blob; std::vector<int64_t> offs{0};
            for (const auto& sp : specials_) { ids.push_back(sp.second); blob += sp.first; offs.push_back(static_cast<int64_t>(blob.size())); }
            const tkz_status r = tkz_encoder_set_special_tokens(enc_, ids.data(), reinterpret_cast<const uint8_t*>(blob.data()), offs.data(), static_cast<int32_t>(ids.size()));
            if (r != TKZ_OK) { tkz_encoder_destroy(enc_); enc_ = nullptr; check(r); }
        }
    }
    ~TikTokenizer() { tkz_encoder_destroy(enc_); }
    TikTokenizer(const TikTokenizer&) = delete;
    TikTokenizer& operator=(const TikTokenizer&) = delete;

    // Encode(string text, IReadOnlyCollection<string> allowedSpecial)        TikTokenizer.cs:178-185
    // With special tokens allowed: ONE call of the single-text special entry (tkz_encode_special_utf8: one kernel launch for a prompt).  Only a registered set
    // the device path does not hold (TKZ_E_UNSUPPORTED) is segmented here, as EncodeBatch does it.
    std::vector<int32_t> Encode(const std::string& text, const std::vector<std::string>& allowedSpecial) const {
        std::vector<int32_t> ids;
        if (encode_special_single(text, allowedSpecial, ids)) return ids;
        return EncodeBatch({text}, allowedSpecial)[0];
    }
    // Encode(string text, bool applySpecialTokens = true)                     TikTokenizer.cs:193-207
    std::vector<int32_t> Encode(const std::string& text, bool applySpecialTokens = true) const {
        if (applySpecialTokens && !specials_.empty()) return Encode(text, all_specials());
        return EncodeBatch({text}, applySpecialTokens)[0];
    }
    std::vector<std::vector<int32_t>> EncodeBatch(const std::vector<std::string>& texts, bool applySpecialTokens = true) const {
        std::vector<std::string> all;
        if (applySpecialTokens) for (const auto& s : specials_) all.push_back(s.first);
        return EncodeBatch(texts, all);
    }
    std::vector<std::vector<int32_t>> EncodeBatch(const std::vector<std::string>& texts, const std::vector<std::string>& allowedSpecial) const {
        struct Item { size_t text; int32_t special; int64_t segment; };
        std::vector<Item> plan;
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (size_t t = 0; t < texts.size(); ++t) {
            for (const Segment& g : segments(texts[t], allowedSpecial)) {
                if (g.special) { plan.push_back({t, g.id, -1}); continue; }
                plan.push_back({t, 0, static_cast<int64_t>(offs.size()) - 1});
                bytes.insert(bytes.end(), texts[t].begin() + g.begin, texts[t].begin() + g.end);
                offs.push_back(static_cast<int64_t>(bytes.size()));
            }
        }
        const int64_t nseg = static_cast<int64_t>(offs.size()) - 1;
        std::vector<int32_t> ids(bytes.size() ? bytes.size() : 1);
        std::vector<int64_t> ooff(static_cast<size_t>(nseg) + 1, 0);
        int64_t needed = 0;
        if (bytes.empty()) bytes.push_back(0);
        check(tkz_encode_batch_utf8(enc_, bytes.data(), offs.data(), nseg, ids.data(), static_cast<int64_t>(ids.size()), ooff.data(), &needed));
        std::vector<std::vector<int32_t>> out(texts.size());
        for (const Item& it : plan) {
            if (it.segment < 0) { out[it.text].push_back(it.special); continue; }
            out[it.text].insert(out[it.text].end(), ids.begin() + ooff[it.segment], ids.begin() + ooff[it.segment + 1]);
        }
        return out;
    }

    // EncodeBatch without a vector per text (FlatBatch above).  The texts are gathered into page-locked memory by `threads` host threads
    // (0: as many as the batch is worth, at most 8), encoded by ONE tkz_encode_batch_utf8 call that reads and writes page-locked buffers,
    // and -- when no special token applies, the reference's plain path (TikTokenizer.cs:180-183,196-199) -- the views of `out` are the
    // call's own output, untouched.
    void EncodeBatchFlat(const std::vector<std::string>& texts, FlatBatch& out, bool applySpecialTokens = true, int threads = 0) const {
        EncodeBatchFlat(texts, applySpecialTokens ? all_specials() : std::vector<std::string>{}, out, threads);
    }
    void EncodeBatchFlat(const std::vector<std::string>& texts, const std::vector<std::string>& allowedSpecial, FlatBatch& out, int threads = 0) const {
        const bool plain = allowedSpecial.empty() || specials_.empty();
        out.n_texts_ = static_cast<int64_t>(texts.size());
        if (plain) {                                           // one segment per text, the texts themselves
            encode_segments(static_cast<int64_t>(texts.size()), [&](int64_t i) { return std::pair<const char*, size_t>(texts[static_cast<size_t>(i)].data(), texts[static_cast<size_t>(i)].size()); }, out, threads);
            out.ids_ = out.out_ids_.as<int32_t>(); out.offsets_ = out.out_offs_.as<int64_t>();
            return;
        }
        // The device cuts the allowed literals out itself (tkz_encode_batch_special_utf8): the whole texts through the same gather as the plain path, the
        // result left in the page-locked buffers.  Only a registered set the device path does not hold (TKZ_E_UNSUPPORTED) is segmented here and spliced.
        if (!special_on_host_) {
            std::vector<int32_t> index;
            for (size_t i = 0; i < specials_.size(); ++i)
                for (const auto& a : allowedSpecial) if (a == specials_[i].first) { index.push_back(static_cast<int32_t>(i)); break; }
            if (encode_segments(static_cast<int64_t>(texts.size()), [&](int64_t i) { return std::pair<const char*, size_t>(texts[static_cast<size_t>(i)].data(), texts[static_cast<size_t>(i)].size()); }, out, threads, &index)) {
                out.ids_ = out.out_ids_.as<int32_t>(); out.offsets_ = out.out_offs_.as<int64_t>();
                return;
            }
            special_on_host_ = true;
        }
        // what goes to the device: (source pointer, length) of every plain segment, and where the special ids go
        struct Item { size_t text; int32_t special; int64_t segment; };
        std::vector<Item> plan;
        std::vector<std::pair<const char*, size_t>> segs;
        for (size_t t = 0; t < texts.size(); ++t)
            for (const Segment& g : segments(texts[t], allowedSpecial)) {
                if (g.special) { plan.push_back({t, g.id, -1}); continue; }
                plan.push_back({t, 0, static_cast<int64_t>(segs.size())});
                segs.emplace_back(texts[t].data() + g.begin, g.end - g.begin);
            }
        const int64_t nseg = static_cast<int64_t>(segs.size());
        encode_segments(nseg, [&](int64_t i) { return segs[static_cast<size_t>(i)]; }, out, threads);
        const int32_t* ids = out.out_ids_.as<int32_t>();
        const int64_t* ooff = out.out_offs_.as<int64_t>();
        // splice the special ids in between the segments' id ranges
        size_t nspecial = 0;
        for (const Item& it : plan) if (it.segment < 0) ++nspecial;
        out.spliced_ids_.resize(static_cast<size_t>(ooff[nseg]) + nspecial);
        out.spliced_offs_.assign(texts.size() + 1, 0);
        int64_t w = 0; size_t cur = 0;
        for (const Item& it : plan) {
            while (cur < it.text) out.spliced_offs_[++cur] = w;
            if (it.segment < 0) { out.spliced_ids_[static_cast<size_t>(w++)] = it.special; continue; }
            const int64_t n = ooff[it.segment + 1] - ooff[it.segment];
            std::memcpy(out.spliced_ids_.data() + w, ids + ooff[it.segment], static_cast<size_t>(n) * 4);
            w += n;
        }
        while (cur < texts.size()) out.spliced_offs_[++cur] = w;
        out.ids_ = out.spliced_ids_.data(); out.offsets_ = out.spliced_offs_.data();
    }

    // The same for hosts whose strings are UTF-16 (a .NET `string`, Java, JavaScript): the plain path (no special tokens applied) on code units --
    // what bindings/csharp/GpuTikTokenizer.EncodeBatchFlat does with `string.CopyTo` + tkz_encode_batch_utf16.  The units are gathered into
    // page-locked memory by `threads` host threads, uploaded as they are (the library cuts the batch into chunks and runs Encoding.UTF8.GetBytes
    // -- TikTokenizer.cs:261 -- on the device while the next chunk is on its way) and the ids come back into page-locked memory.
    void EncodeBatchFlatUtf16(const std::vector<std::u16string>& texts, FlatBatch& out, int threads = 0) const { (void)flat_utf16(texts, out, threads, nullptr); }
    // allowed: null, or the indices of the allowed special tokens (tkz_encode_batch_special_utf16); false (nothing encoded): that entry refused the registered set
    bool flat_utf16(const std::vector<std::u16string>& texts, FlatBatch& out, int threads, const std::vector<int32_t>* allowed) const {
        const int64_t n = static_cast<int64_t>(texts.size());
        out.n_texts_ = n;
        int nth = threads > 0 ? threads : static_cast<int>(std::min<int64_t>(16, n >> 14));
        const unsigned hw = std::thread::hardware_concurrency();
        if (hw && nth > static_cast<int>(hw)) nth = static_cast<int>(hw);
        if (nth < 1) nth = 1;
        int64_t* offs = static_cast<int64_t*>(out.in_offs_.ensure((static_cast<size_t>(n) + 1) * 8));
        offs[0] = 0;
        for (int64_t i = 0; i < n; ++i) offs[i + 1] = offs[i] + static_cast<int64_t>(texts[static_cast<size_t>(i)].size());
        const int64_t total = offs[n];
        uint16_t* units = static_cast<uint16_t*>(out.in_bytes_.ensure(static_cast<size_t>(total) * 2 + 64));
        {
            Joiner j;
            for (int t = 0; t < nth; ++t)
                j.pool.emplace_back([&, t] {
                    const int64_t lo = t == 0 ? 0 : std::lower_bound(offs, offs + n, total / nth * t) - offs;
                    const int64_t hi = t == nth - 1 ? n : std::lower_bound(offs, offs + n, total / nth * (t + 1)) - offs;
                    for (int64_t i = lo; i < hi; ++i) std::memcpy(units + offs[i], texts[static_cast<size_t>(i)].data(), texts[static_cast<size_t>(i)].size() * 2);
                });
        }
        int64_t* ooff = static_cast<int64_t*>(out.out_offs_.ensure((static_cast<size_t>(n) + 1) * 8));
        // a code unit is at most three UTF-8 bytes and a token at least one byte: 3 * total ids always suffice; text has a token per ~4 units, so the
        // first call gets room for one per two and the call is repeated with the exact count when that was not enough
        int64_t cap = std::max<int64_t>(1, std::min<int64_t>(3 * total, std::max<int64_t>(total / 2 + 4096, static_cast<int64_t>(static_cast<double>(total) * out.tokens_per_byte_ * 1.1))));
        for (;;) {
            int32_t* ids = static_cast<int32_t*>(out.out_ids_.ensure(static_cast<size_t>(cap) * 4));
            int64_t needed = 0;
            const tkz_status st = allowed ? tkz_encode_batch_special_utf16(enc_, units, offs, n, allowed->data(), static_cast<int32_t>(allowed->size()), ids, cap, ooff, &needed)
                                          : tkz_encode_batch_utf16(enc_, units, offs, n, ids, cap, ooff, &needed);
            if (allowed && st == TKZ_E_UNSUPPORTED) return false;
            if (st == TKZ_E_CAPACITY && needed > cap) { cap = needed; continue; }
            check(st);
            if (total > 0) out.tokens_per_byte_ = std::max(out.tokens_per_byte_, static_cast<double>(needed) / static_cast<double>(total));
            break;
        }
        out.ids_ = out.out_ids_.as<int32_t>(); out.offsets_ = out.out_offs_.as<int64_t>();
        return true;
    }

    using Trimmed = std::pair<std::vector<int32_t>, std::string>;   // (List<int> TokenIds, string Text)
    // EncodeTrimSuffix(string, IReadOnlyCollection<string> allowedSpecial, int maxTokenCount)     TikTokenizer.cs:394-403
    // (one string: tkz_encode_trim_utf8, the single-text trim entry -- one kernel launch for a prompt; the host walk where the batch methods take it)
    Trimmed EncodeTrimSuffix(const std::string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        Trimmed out;
        return trim_one_device(text, allowedSpecial, maxTokenCount, TKZ_TRIM_SUFFIX, out) ? out : trim_suffix_host(text, allowedSpecial, maxTokenCount);
    }
    // EncodeTrimSuffix / EncodeTrimPrefix for a batch of texts: ONE device call (tkz_encode_batch_trim_utf8 -- the literals cut out, the pieces counted, the
    // cut chosen and the kept ids compacted on the device; the text is sliced at the cut's byte position).  The host walk over piece_items() below remains for
    // a registered set the device path does not hold (TKZ_E_UNSUPPORTED) and for a negative maximum (the reference's prefix variant returns the whole text then).
    std::vector<Trimmed> EncodeTrimSuffixBatch(const std::vector<std::string>& texts, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        std::vector<Trimmed> out;
        if (trim_batch_device(texts, allowedSpecial, maxTokenCount, TKZ_TRIM_SUFFIX, out)) return out;
        for (const std::string& t : texts) out.push_back(trim_suffix_host(t, allowedSpecial, maxTokenCount));
        return out;
    }
    std::vector<Trimmed> EncodeTrimSuffixBatch(const std::vector<std::string>& texts, int maxTokenCount, bool applySpecialTokens = true) const {
        return EncodeTrimSuffixBatch(texts, applySpecialTokens ? all_specials() : std::vector<std::string>{}, maxTokenCount);
    }
    std::vector<Trimmed> EncodeTrimPrefixBatch(const std::vector<std::string>& texts, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        std::vector<Trimmed> out;
        if (trim_batch_device(texts, allowedSpecial, maxTokenCount, TKZ_TRIM_PREFIX, out)) return out;
        for (const std::string& t : texts) out.push_back(trim_prefix_host(t, allowedSpecial, maxTokenCount));
        return out;
    }
    std::vector<Trimmed> EncodeTrimPrefixBatch(const std::vector<std::string>& texts, int maxTokenCount, bool applySpecialTokens = true) const {
        return EncodeTrimPrefixBatch(texts, applySpecialTokens ? all_specials() : std::vector<std::string>{}, maxTokenCount);
    }
    Trimmed trim_suffix_host(const std::string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        std::vector<int32_t> ids;
        int64_t tokenCount = 0; size_t encodeLength = 0;
        for (const PieceItem& it : piece_items(text, allowedSpecial)) {            // the walk of :288-341 / :343-392
            tokenCount += static_cast<int64_t>(it.ids.size());
            if (tokenCount > maxTokenCount) break;                                // the piece that overflows is dropped, with all after it
            ids.insert(ids.end(), it.ids.begin(), it.ids.end());
            encodeLength = it.end;
            if (tokenCount >= maxTokenCount) break;
        }
        return {ids, text.substr(0, encodeLength)};
    }
    // EncodeTrimSuffix(string, int maxTokenCount, bool applySpecialTokens = true)                  TikTokenizer.cs:412-429
    Trimmed EncodeTrimSuffix(const std::string& text, int maxTokenCount, bool applySpecialTokens = true) const {
        return EncodeTrimSuffix(text, applySpecialTokens ? all_specials() : std::vector<std::string>{}, maxTokenCount);
    }
    // EncodeTrimPrefix(string, IReadOnlyCollection<string> allowedSpecial, int maxTokenCount)     TikTokenizer.cs:529-536
    Trimmed EncodeTrimPrefix(const std::string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        Trimmed out;
        return trim_one_device(text, allowedSpecial, maxTokenCount, TKZ_TRIM_PREFIX, out) ? out : trim_prefix_host(text, allowedSpecial, maxTokenCount);
    }
    Trimmed trim_prefix_host(const std::string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        std::vector<int32_t> ids;
        std::vector<std::pair<int64_t, size_t>> boundaries{{0, 0}};               // tokenCountMap (:438-441)
        int64_t tokenCount = 0;
        for (const PieceItem& it : piece_items(text, allowedSpecial)) {
            tokenCount += static_cast<int64_t>(it.ids.size());
            ids.insert(ids.end(), it.ids.begin(), it.ids.end());
            boundaries.push_back({tokenCount, it.end});
        }
        if (tokenCount <= maxTokenCount) return {ids, text};                      // TrimPrefix (:470-483)
        const int64_t prefix = tokenCount - maxTokenCount;
        int64_t cutTokens = 0; size_t cutLen = 0;
        for (const auto& b : boundaries) if (b.first >= prefix) { cutTokens = b.first; cutLen = b.second; break; }
        return {std::vector<int32_t>(ids.begin() + cutTokens, ids.end()), text.substr(cutLen)};
    }
    // EncodeTrimPrefix(string, int maxTokenCount, bool applySpecialTokens = true)                  TikTokenizer.cs:545-564
    Trimmed EncodeTrimPrefix(const std::string& text, int maxTokenCount, bool applySpecialTokens = true) const {
        return EncodeTrimPrefix(text, applySpecialTokens ? all_specials() : std::vector<std::string>{}, maxTokenCount);
    }
    // a batch of UTF-16 strings (plain path): the code units go to the device as they are (tkz_encode_batch_utf16)
    std::vector<std::vector<int32_t>> EncodeBatchUtf16(const std::vector<std::u16string>& texts) const {
        std::vector<uint16_t> units;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { units.insert(units.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(units.size())); }
        const size_t cap = units.size() * 3 + 1;
        std::vector<int32_t> ids(cap);
        std::vector<int64_t> ooff(texts.size() + 1, 0);
        int64_t needed = 0;
        if (units.empty()) units.push_back(0);
        check(tkz_encode_batch_utf16(enc_, units.data(), offs.data(), static_cast<int64_t>(texts.size()), ids.data(), static_cast<int64_t>(cap), ooff.data(), &needed));
        std::vector<std::vector<int32_t>> out(texts.size());
        for (size_t t = 0; t < texts.size(); ++t) out[t].assign(ids.begin() + ooff[t], ids.begin() + ooff[t + 1]);
        return out;
    }
    // the code units of a .NET string; plain path only (Encode(text, false))
    std::vector<int32_t> EncodeUtf16(const std::u16string& text) const {
        std::vector<int32_t> ids(text.size() * 3 + 1);
        int64_t n = 0;
        check(tkz_encode_utf16(enc_, reinterpret_cast<const uint16_t*>(text.data()), static_cast<int64_t>(text.size()), ids.data(),
                               static_cast<int64_t>(ids.size()), &n));
        ids.resize(static_cast<size_t>(n));
        return ids;
    }
    // ---- std::u16string callers: special tokens and trimming on the code units themselves (tkz_encode_batch_special_utf16 / tkz_encode_batch_trim_utf16) ----
    // The device transcodes, and searches the literals as .NET searches the string: a lone surrogate is not U+FFFD.  With a registered set the device path does
    // not hold (TKZ_E_UNSUPPORTED), and for a negative maximum, the host walk over piece_items16() below does the work, as the UTF-8 methods' does.
    using Trimmed16 = std::pair<std::vector<int32_t>, std::u16string>;
    void EncodeBatchFlatUtf16(const std::vector<std::u16string>& texts, bool applySpecialTokens, FlatBatch& out, int threads = 0) const {
        EncodeBatchFlatUtf16(texts, applySpecialTokens ? all_specials() : std::vector<std::string>{}, out, threads);
    }
    void EncodeBatchFlatUtf16(const std::vector<std::u16string>& texts, const std::vector<std::string>& allowedSpecial, FlatBatch& out, int threads = 0) const {
        if (allowedSpecial.empty() || specials_.empty()) { EncodeBatchFlatUtf16(texts, out, threads); return; }
        if (!special_on_host_) {
            const std::vector<int32_t> index = allowed_index(allowedSpecial);
            if (flat_utf16(texts, out, threads, &index)) return;
            special_on_host_ = true;
        }
        out.n_texts_ = static_cast<int64_t>(texts.size());
        out.spliced_ids_.clear();
        out.spliced_offs_.assign(1, 0);
        for (const std::u16string& t : texts) {
            const std::vector<int32_t> ids = encode_host16(t, allowedSpecial);
            out.spliced_ids_.insert(out.spliced_ids_.end(), ids.begin(), ids.end());
            out.spliced_offs_.push_back(static_cast<int64_t>(out.spliced_ids_.size()));
        }
        out.ids_ = out.spliced_ids_.data(); out.offsets_ = out.spliced_offs_.data();
    }
    std::vector<std::vector<int32_t>> EncodeBatchUtf16(const std::vector<std::u16string>& texts, const std::vector<std::string>& allowedSpecial) const {
        FlatBatch fb;
        EncodeBatchFlatUtf16(texts, allowedSpecial, fb, 1);
        std::vector<std::vector<int32_t>> out(texts.size());
        for (size_t t = 0; t < texts.size(); ++t) out[t] = fb.text(static_cast<int64_t>(t));
        return out;
    }
    // (one string: tkz_encode_special_utf16, the single-text special entry)
    std::vector<int32_t> EncodeUtf16(const std::u16string& text, const std::vector<std::string>& allowedSpecial) const {
        if (!allowedSpecial.empty() && !specials_.empty() && !special_on_host_) {
            const std::vector<int32_t> index = allowed_index(allowedSpecial);
            std::vector<int32_t> ids(text.size() * 3 + 1);
            int64_t n = 0;
            const tkz_status st = tkz_encode_special_utf16(enc_, reinterpret_cast<const uint16_t*>(text.data()), static_cast<int64_t>(text.size()), index.data(),
                                                           static_cast<int32_t>(index.size()), ids.data(), static_cast<int64_t>(ids.size()), &n);
            if (st != TKZ_E_UNSUPPORTED) { check(st); ids.resize(static_cast<size_t>(n)); return ids; }
            special_on_host_ = true;
        }
        return EncodeBatchUtf16({text}, allowedSpecial)[0];
    }
    // ---- counts: Encode(...).Count without the ids (tkz_count_utf8 / _utf16, tkz_count_batch_utf8 / _utf16: no id buffer, only the offsets come back) ----
    // The count of every text is the size of what the Encode method of the same arguments returns.  With a registered set the device path does not hold
    // (TKZ_E_UNSUPPORTED) it IS that size: the host segmentation encodes.
    int64_t CountTokens(const std::string& text, const std::vector<std::string>& allowedSpecial) const {
        const bool plain = allowedSpecial.empty() || specials_.empty();
        if (plain || !special_on_host_) {
            const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
            const uint8_t zero = 0;
            int64_t n = 0;
            const tkz_status st = tkz_count_utf8(enc_, text.empty() ? &zero : reinterpret_cast<const uint8_t*>(text.data()), static_cast<int64_t>(text.size()),
                                                 index.data(), static_cast<int32_t>(index.size()), &n);
            if (st != TKZ_E_UNSUPPORTED) { check(st); return n; }
            special_on_host_ = true;
        }
        return static_cast<int64_t>(Encode(text, allowedSpecial).size());
    }
    int64_t CountTokens(const std::string& text, bool applySpecialTokens = true) const {
        return CountTokens(text, applySpecialTokens ? all_specials() : std::vector<std::string>{});
    }
    std::vector<int64_t> CountTokensBatch(const std::vector<std::string>& texts, const std::vector<std::string>& allowedSpecial) const {
        std::vector<int64_t> counts(texts.size(), 0);
        if (texts.empty()) return counts;
        const bool plain = allowedSpecial.empty() || specials_.empty();
        if (plain || !special_on_host_) {
            std::vector<uint8_t> bytes;
            std::vector<int64_t> offs{0}, ooff(texts.size() + 1, 0);
            for (const auto& t : texts) { bytes.insert(bytes.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(bytes.size())); }
            if (bytes.empty()) bytes.push_back(0);
            const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
            const tkz_status st = tkz_count_batch_utf8(enc_, bytes.data(), offs.data(), static_cast<int64_t>(texts.size()), index.data(), static_cast<int32_t>(index.size()),
                                                       ooff.data(), nullptr);
            if (st != TKZ_E_UNSUPPORTED) {
                check(st);
                for (size_t t = 0; t < texts.size(); ++t) counts[t] = ooff[t + 1] - ooff[t];
                return counts;
            }
            special_on_host_ = true;
        }
        const std::vector<std::vector<int32_t>> ids = EncodeBatch(texts, allowedSpecial);
        for (size_t t = 0; t < texts.size(); ++t) counts[t] = static_cast<int64_t>(ids[t].size());
        return counts;
    }
    std::vector<int64_t> CountTokensBatch(const std::vector<std::string>& texts, bool applySpecialTokens = true) const {
        return CountTokensBatch(texts, applySpecialTokens ? all_specials() : std::vector<std::string>{});
    }
    // ... the code units of .NET strings: the batch is transcoded on the device, the one text on the host (as EncodeBatchUtf16 / EncodeUtf16 have it)
    int64_t CountTokensUtf16(const std::u16string& text, const std::vector<std::string>& allowedSpecial = {}) const {
        const bool plain = allowedSpecial.empty() || specials_.empty();
        if (plain || !special_on_host_) {
            const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
            const uint16_t zero = 0;
            int64_t n = 0;
            const tkz_status st = tkz_count_utf16(enc_, text.empty() ? &zero : reinterpret_cast<const uint16_t*>(text.data()), static_cast<int64_t>(text.size()),
                                                  index.data(), static_cast<int32_t>(index.size()), &n);
            if (st != TKZ_E_UNSUPPORTED) { check(st); return n; }
            special_on_host_ = true;
        }
        return static_cast<int64_t>(EncodeUtf16(text, allowedSpecial).size());
    }
    std::vector<int64_t> CountTokensBatchUtf16(const std::vector<std::u16string>& texts, const std::vector<std::string>& allowedSpecial = {}) const {
        std::vector<int64_t> counts(texts.size(), 0);
        if (texts.empty()) return counts;
        const bool plain = allowedSpecial.empty() || specials_.empty();
        if (plain || !special_on_host_) {
            std::vector<uint16_t> units;
            std::vector<int64_t> offs{0}, ooff(texts.size() + 1, 0);
            for (const auto& t : texts) { units.insert(units.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(units.size())); }
            if (units.empty()) units.push_back(0);
            const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
            const tkz_status st = tkz_count_batch_utf16(enc_, units.data(), offs.data(), static_cast<int64_t>(texts.size()), index.data(), static_cast<int32_t>(index.size()),
                                                        ooff.data(), nullptr);
            if (st != TKZ_E_UNSUPPORTED) {
                check(st);
                for (size_t t = 0; t < texts.size(); ++t) counts[t] = ooff[t + 1] - ooff[t];
                return counts;
            }
            special_on_host_ = true;
        }
        const std::vector<std::vector<int32_t>> ids = EncodeBatchUtf16(texts, allowedSpecial);
        for (size_t t = 0; t < texts.size(); ++t) counts[t] = static_cast<int64_t>(ids[t].size());
        return counts;
    }
    // ---- token spans: Encode, and where every token's text starts (tkz_encode_spans_utf8 / _utf16, tkz_encode_batch_spans_utf8 / _utf16) ----
    // std::string: offsets in BYTES of the text, whose spans are exactly the tokens' keys; std::u16string: offsets in CODE UNITS -- a token that starts inside a
    // character starts after that character's units, one of continuation bytes only has an empty span (tkz.h).  Token t is [starts[t], starts[t + 1]), the last
    // one ends at the text's length.  A registered set the device's special entries do not hold is a NotImplementedError here: there is no host path.
    struct TokenSpans { std::vector<int32_t> ids; std::vector<int32_t> starts; };
    TokenSpans EncodeWithOffsets(const std::string& text, const std::vector<std::string>& allowedSpecial = {}) const {
        return std::move(EncodeWithOffsetsBatch(std::vector<std::string>{text}, allowedSpecial)[0]);
    }
    std::vector<TokenSpans> EncodeWithOffsetsBatch(const std::vector<std::string>& texts, const std::vector<std::string>& allowedSpecial = {}) const {
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { bytes.insert(bytes.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(bytes.size())); }
        return spans_batch<uint8_t>(bytes, offs, allowedSpecial, false);
    }
    TokenSpans EncodeWithOffsetsUtf16(const std::u16string& text, const std::vector<std::string>& allowedSpecial = {}) const {
        return std::move(EncodeWithOffsetsBatchUtf16(std::vector<std::u16string>{text}, allowedSpecial)[0]);
    }
    std::vector<TokenSpans> EncodeWithOffsetsBatchUtf16(const std::vector<std::u16string>& texts, const std::vector<std::string>& allowedSpecial = {}) const {
        std::vector<uint16_t> units;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { units.insert(units.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(units.size())); }
        return spans_batch<uint16_t>(units, offs, allowedSpecial, true);
    }
    // ---- token-budget chunks: the repeated-EncodeTrimSuffix loop in ONE call (tkz_encode_batch_chunks_utf8 / _utf16; tkz.h states the rule) ----
    // A list of (ids, text) per text: chunks of at most maxTokenCount tokens that end at piece boundaries where one is in reach; a piece of more tokens than the
    // budget is cut into runs of maxTokenCount.  The ids concatenate to Encode's and the texts to the input.  std::string: the texts are sliced at the chunks' BYTE
    // starts, so a chunk may begin inside a character; std::u16string: at their starts in CODE UNITS -- a character cut by a chunk boundary goes to the earlier
    // chunk.  maxTokenCount < 1 is the C ABI's TKZ_E_ARG.  A registered set the device's special entries do not hold is a NotImplementedError here: there is
    // no host path.
    std::vector<Trimmed> EncodeChunks(const std::string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        return std::move(EncodeChunksBatch(std::vector<std::string>{text}, allowedSpecial, maxTokenCount)[0]);
    }
    std::vector<Trimmed> EncodeChunks(const std::string& text, int maxTokenCount, bool applySpecialTokens = true) const {
        return EncodeChunks(text, applySpecialTokens ? all_specials() : std::vector<std::string>{}, maxTokenCount);
    }
    std::vector<std::vector<Trimmed>> EncodeChunksBatch(const std::vector<std::string>& texts, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { bytes.insert(bytes.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(bytes.size())); }
        return chunks_batch<uint8_t, std::string>(bytes, offs, texts, allowedSpecial, maxTokenCount, false);
    }
    std::vector<std::vector<Trimmed>> EncodeChunksBatch(const std::vector<std::string>& texts, int maxTokenCount, bool applySpecialTokens = true) const {
        return EncodeChunksBatch(texts, applySpecialTokens ? all_specials() : std::vector<std::string>{}, maxTokenCount);
    }
    using Chunk16 = std::pair<std::vector<int32_t>, std::u16string>;
    std::vector<Chunk16> EncodeChunksUtf16(const std::u16string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        return std::move(EncodeChunksBatchUtf16(std::vector<std::u16string>{text}, allowedSpecial, maxTokenCount)[0]);
    }
    std::vector<std::vector<Chunk16>> EncodeChunksBatchUtf16(const std::vector<std::u16string>& texts, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        std::vector<uint16_t> units;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { units.insert(units.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(units.size())); }
        return chunks_batch<uint16_t, std::u16string>(units, offs, texts, allowedSpecial, maxTokenCount, true);
    }
    // ---- overlapping token-budget chunks: a chunk size and an overlap (tkz_encode_batch_chunks_overlap_utf8 / _utf16; tkz.h states the rule) ----
    // EncodeChunks with 0 <= overlap < maxTokenCount (anything else is the C ABI's TKZ_E_ARG): consecutive chunks share at most `overlap` tokens and the text of
    // those tokens.  A chunk is what EncodeTrimSuffix(rest, maxTokenCount) returns, the next one starts with what EncodeTrimPrefix(chunk text, overlap) keeps (one
    // item further on when that is the whole chunk, behind the chunk when a chunk begun there would end where this one does).  The texts are slices of the input
    // [start, end): bytes for std::string, code units for std::u16string.  overlap 0 gives EncodeChunks' result.  No host path, as EncodeChunks.
    std::vector<Trimmed> EncodeChunksOverlap(const std::string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount, int overlap) const {
        return std::move(EncodeChunksOverlapBatch(std::vector<std::string>{text}, allowedSpecial, maxTokenCount, overlap)[0]);
    }
    std::vector<Trimmed> EncodeChunksOverlap(const std::string& text, int maxTokenCount, int overlap, bool applySpecialTokens = true) const {
        return EncodeChunksOverlap(text, applySpecialTokens ? all_specials() : std::vector<std::string>{}, maxTokenCount, overlap);
    }
    std::vector<std::vector<Trimmed>> EncodeChunksOverlapBatch(const std::vector<std::string>& texts, const std::vector<std::string>& allowedSpecial, int maxTokenCount,
                                                               int overlap) const {
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { bytes.insert(bytes.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(bytes.size())); }
        return chunks_overlap_batch<uint8_t, std::string>(bytes, offs, texts, allowedSpecial, maxTokenCount, overlap, false);
    }
    std::vector<std::vector<Trimmed>> EncodeChunksOverlapBatch(const std::vector<std::string>& texts, int maxTokenCount, int overlap, bool applySpecialTokens = true) const {
        return EncodeChunksOverlapBatch(texts, applySpecialTokens ? all_specials() : std::vector<std::string>{}, maxTokenCount, overlap);
    }
    std::vector<Chunk16> EncodeChunksOverlapUtf16(const std::u16string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount, int overlap) const {
        return std::move(EncodeChunksOverlapBatchUtf16(std::vector<std::u16string>{text}, allowedSpecial, maxTokenCount, overlap)[0]);
    }
    std::vector<std::vector<Chunk16>> EncodeChunksOverlapBatchUtf16(const std::vector<std::u16string>& texts, const std::vector<std::string>& allowedSpecial,
                                                                    int maxTokenCount, int overlap) const {
        std::vector<uint16_t> units;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { units.insert(units.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(units.size())); }
        return chunks_overlap_batch<uint16_t, std::u16string>(units, offs, texts, allowedSpecial, maxTokenCount, overlap, true);
    }
    // ---- packed rows: BOS / EOS framing, rows of the context length, positions and segment starts in ONE call (tkz_encode_batch_packed_utf8 / _utf16) ----
    // Every text's ids -- Encode's for the same arguments -- with bos in front and eos behind it (-1: none; any id >= 0 is taken as it is), the stream cut into
    // rows of rowLen and padded with pad.  ids and pos are n_rows * rowLen entries, row-major; pos restarts at every document and every row; seg_starts
    // (cu_seqlens) holds the segment starts and ends with the stream's length; doc_offsets[d] is where text d starts in the stream (tkz.h states the rule).
    // A registered set the device's special entries do not hold is a NotImplementedError here: there is no host path.
    struct PackedRows { int64_t row_len = 0, n_rows = 0, total_tokens = 0; std::vector<int32_t> ids, pos; std::vector<int64_t> seg_starts, doc_offsets; };
    PackedRows EncodeBatchPacked(const std::vector<std::string>& texts, int64_t rowLen, const std::vector<std::string>& allowedSpecial = {}, int32_t bos = -1, int32_t eos = -1,
                                 int32_t pad = 0) const {
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { bytes.insert(bytes.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(bytes.size())); }
        return packed_batch<uint8_t>(bytes, offs, rowLen, allowedSpecial, bos, eos, pad, false);
    }
    PackedRows EncodeBatchPacked(const std::vector<std::u16string>& texts, int64_t rowLen, const std::vector<std::string>& allowedSpecial = {}, int32_t bos = -1, int32_t eos = -1,
                                 int32_t pad = 0) const {
        std::vector<uint16_t> units;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { units.insert(units.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(units.size())); }
        return packed_batch<uint16_t>(units, offs, rowLen, allowedSpecial, bos, eos, pad, true);
    }
    // ---- padded rows: truncation, framing, padding to a common width and the attention mask in ONE call (tkz_encode_batch_padded_utf8 / _utf16) ----
    // Every text's ids -- Encode's for the same arguments -- cut to maxLength less the framing (cutSide TKZ_TRIM_SUFFIX keeps the head, TKZ_TRIM_PREFIX the tail), with
    // bos in front and eos behind what is kept (-1: none; any id >= 0 is taken as it is), a row a text, padded with pad on padSide to the longest row rounded up to
    // padMultiple -- at most maxLength; padMultiple 0: to maxLength itself.  ids, mask (1 on content) and pos (the index inside the content) are n * width entries,
    // row-major; lens the content lengths; n_cut the texts that were cut; total_tokens the uncut total (tkz.h states the rule).  The cut is a plain cut of the id
    // list, not EncodeTrimSuffix's whole-item cut.  A registered set the device's special entries do not hold is a NotImplementedError here: there is no host path.
    struct PaddedRows { int64_t width = 0, total_tokens = 0, n_cut = 0; std::vector<int32_t> ids, pos, lens; std::vector<uint8_t> mask; };
    PaddedRows EncodeBatchPadded(const std::vector<std::string>& texts, int64_t maxLength, const std::vector<std::string>& allowedSpecial = {}, int32_t bos = -1, int32_t eos = -1,
                                 int32_t pad = 0, tkz_trim_side cutSide = TKZ_TRIM_SUFFIX, tkz_pad_side padSide = TKZ_PAD_RIGHT, int64_t padMultiple = 1) const {
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { bytes.insert(bytes.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(bytes.size())); }
        return padded_batch<uint8_t>(bytes, offs, maxLength, allowedSpecial, bos, eos, pad, cutSide, padSide, padMultiple, false);
    }
    PaddedRows EncodeBatchPadded(const std::vector<std::u16string>& texts, int64_t maxLength, const std::vector<std::string>& allowedSpecial = {}, int32_t bos = -1, int32_t eos = -1,
                                 int32_t pad = 0, tkz_trim_side cutSide = TKZ_TRIM_SUFFIX, tkz_pad_side padSide = TKZ_PAD_RIGHT, int64_t padMultiple = 1) const {
        std::vector<uint16_t> units;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { units.insert(units.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(units.size())); }
        return padded_batch<uint16_t>(units, offs, maxLength, allowedSpecial, bos, eos, pad, cutSide, padSide, padMultiple, true);
    }
    // ---- length-bucketed padded rows: the padded rows of the texts sorted by length, every bucket of bucketRows rows at its own width, in ONE call
    // (tkz_encode_batch_bucketed_utf8 / _utf16) ----
    // EncodeBatchPadded's arguments and two more: bucketRows (1 .. 2^31 - 1) and order.  The texts are sorted by their content length -- ascending or descending,
    // equal lengths keep the texts' order --, cut into buckets of bucketRows sorted rows, and every bucket is padded to ITS OWN longest row (rounded up to padMultiple,
    // at most maxLength; padMultiple 0: to maxLength itself).  Bucket b is ids / mask / pos [bucket_offsets[b], bucket_offsets[b + 1]): rows(b) x bucket_widths[b],
    // row-major; its row i is text order[b * bucketRows + i]; rank is the inverse of order; lens are in the texts' order (tkz.h states the rule).
    struct BucketedRows {
        int64_t total_positions = 0, total_tokens = 0, n_cut = 0, bucket_rows = 0;
        std::vector<int32_t> ids, pos, lens, bucket_widths; std::vector<uint8_t> mask; std::vector<int64_t> order, rank, bucket_offsets;
        int64_t buckets() const { return static_cast<int64_t>(bucket_widths.size()); }
        int64_t rows(int64_t b) const { return std::min<int64_t>(bucket_rows, static_cast<int64_t>(order.size()) - b * bucket_rows); }
    };
    BucketedRows EncodeBatchBucketed(const std::vector<std::string>& texts, int64_t maxLength, int64_t bucketRows, tkz_bucket_order order = TKZ_BUCKET_ASCENDING,
                                     const std::vector<std::string>& allowedSpecial = {}, int32_t bos = -1, int32_t eos = -1, int32_t pad = 0,
                                     tkz_trim_side cutSide = TKZ_TRIM_SUFFIX, tkz_pad_side padSide = TKZ_PAD_RIGHT, int64_t padMultiple = 1) const {
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { bytes.insert(bytes.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(bytes.size())); }
        return bucketed_batch<uint8_t>(bytes, offs, maxLength, bucketRows, order, allowedSpecial, bos, eos, pad, cutSide, padSide, padMultiple, false);
    }
    BucketedRows EncodeBatchBucketed(const std::vector<std::u16string>& texts, int64_t maxLength, int64_t bucketRows, tkz_bucket_order order = TKZ_BUCKET_ASCENDING,
                                     const std::vector<std::string>& allowedSpecial = {}, int32_t bos = -1, int32_t eos = -1, int32_t pad = 0,
                                     tkz_trim_side cutSide = TKZ_TRIM_SUFFIX, tkz_pad_side padSide = TKZ_PAD_RIGHT, int64_t padMultiple = 1) const {
        std::vector<uint16_t> units;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { units.insert(units.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(units.size())); }
        return bucketed_batch<uint16_t>(units, offs, maxLength, bucketRows, order, allowedSpecial, bos, eos, pad, cutSide, padSide, padMultiple, true);
    }
    // ---- token-budget buckets: the same sorted rows cut greedily into buckets of at most maxTokens positions (rows x width) and maxRows rows, in ONE call
    // (tkz_encode_batch_budgeted_utf8 / _utf16) ----
    // EncodeBatchBucketed's arguments with maxTokens (maxLength .. 2^62) in front of the row count, which becomes a cap (kNoRowCap: none).  Bucket b holds the sorted
    // rows [bucket_rows[b], bucket_rows[b + 1]) -- texts order[...] -- at ids / mask / pos [bucket_offsets[b], bucket_offsets[b + 1]), rows(b) x bucket_widths[b]
    // (tkz.h states the rule).
    static constexpr int64_t kNoRowCap = INT32_MAX;
    struct BudgetedRows {
        int64_t total_positions = 0, total_tokens = 0, n_cut = 0, n_buckets = 0;
        std::vector<int32_t> ids, pos, lens, bucket_widths; std::vector<uint8_t> mask; std::vector<int64_t> order, rank, bucket_offsets, bucket_rows;
        int64_t buckets() const { return n_buckets; }
        int64_t rows(int64_t b) const { return bucket_rows[static_cast<size_t>(b) + 1] - bucket_rows[static_cast<size_t>(b)]; }
    };
    BudgetedRows EncodeBatchBudgeted(const std::vector<std::string>& texts, int64_t maxLength, int64_t maxTokens, int64_t maxRows = kNoRowCap,
                                     tkz_bucket_order order = TKZ_BUCKET_ASCENDING, const std::vector<std::string>& allowedSpecial = {}, int32_t bos = -1, int32_t eos = -1,
                                     int32_t pad = 0, tkz_trim_side cutSide = TKZ_TRIM_SUFFIX, tkz_pad_side padSide = TKZ_PAD_RIGHT, int64_t padMultiple = 1) const {
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { bytes.insert(bytes.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(bytes.size())); }
        return budgeted_batch<uint8_t>(bytes, offs, maxLength, maxTokens, maxRows, order, allowedSpecial, bos, eos, pad, cutSide, padSide, padMultiple, false);
    }
    BudgetedRows EncodeBatchBudgeted(const std::vector<std::u16string>& texts, int64_t maxLength, int64_t maxTokens, int64_t maxRows = kNoRowCap,
                                     tkz_bucket_order order = TKZ_BUCKET_ASCENDING, const std::vector<std::string>& allowedSpecial = {}, int32_t bos = -1, int32_t eos = -1,
                                     int32_t pad = 0, tkz_trim_side cutSide = TKZ_TRIM_SUFFIX, tkz_pad_side padSide = TKZ_PAD_RIGHT, int64_t padMultiple = 1) const {
        std::vector<uint16_t> units;
        std::vector<int64_t> offs{0};
        for (const auto& t : texts) { units.insert(units.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(units.size())); }
        return budgeted_batch<uint16_t>(units, offs, maxLength, maxTokens, maxRows, order, allowedSpecial, bos, eos, pad, cutSide, padSide, padMultiple, true);
    }
    // ---- pair rows: two texts a row -- [bos] first sep x sepCount second [eos] --, cut to maxLength by a strategy, padded to a common width, in ONE call
    // (tkz_encode_batch_pairs_utf8 / _utf16) ----
    // Row i holds first[i] and second[i]: their ids -- Encode's for the same arguments -- cut to maxLength less the framing by `truncation` (TKZ_PAIR_LONGEST_FIRST: an
    // id at a time from the longer text, from the second on a tie; TKZ_PAIR_ONLY_FIRST; TKZ_PAIR_ONLY_SECOND), cutSide TKZ_TRIM_SUFFIX keeping the heads and
    // TKZ_TRIM_PREFIX the tails, padded with pad on padSide to the longest row rounded up to padMultiple -- at most maxLength; padMultiple 0: to maxLength itself.  ids,
    // mask (1 on content), type_ids (1 on the second text's ids and the eos) and pos are n * width entries, row-major; lens the content lengths; kept the ids kept of
    // either text (2 a row); n_cut the pairs that were cut; total_tokens the uncut total (tkz.h states the rule).  bos, sep, eos: -1 for none (sepCount is 0 then).
    // first and second of different sizes are an Error (TKZ_E_ARG).  A registered set the device's special entries do not hold is a NotImplementedError.
    struct PairRows { int64_t width = 0, total_tokens = 0, n_cut = 0; std::vector<int32_t> ids, pos, lens, kept; std::vector<uint8_t> mask, type_ids; };
    PairRows EncodeBatchPairs(const std::vector<std::string>& first, const std::vector<std::string>& second, int64_t maxLength, const std::vector<std::string>& allowedSpecial = {},
                              int32_t bos = -1, int32_t sep = -1, int32_t sepCount = 1, int32_t eos = -1, int32_t pad = 0, tkz_pair_truncation truncation = TKZ_PAIR_LONGEST_FIRST,
                              tkz_trim_side cutSide = TKZ_TRIM_SUFFIX, tkz_pad_side padSide = TKZ_PAD_RIGHT, int64_t padMultiple = 1) const {
        if (first.size() != second.size()) throw Error(TKZ_E_ARG, "EncodeBatchPairs: first and second must hold as many texts as each other");
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (size_t i = 0; i < first.size(); ++i)
            for (const std::string* t : {&first[i], &second[i]}) { bytes.insert(bytes.end(), t->begin(), t->end()); offs.push_back(static_cast<int64_t>(bytes.size())); }
        return pairs_batch<uint8_t>(bytes, offs, maxLength, allowedSpecial, bos, sep, sepCount, eos, pad, truncation, cutSide, padSide, padMultiple, false);
    }
    PairRows EncodeBatchPairs(const std::vector<std::u16string>& first, const std::vector<std::u16string>& second, int64_t maxLength, const std::vector<std::string>& allowedSpecial = {},
                              int32_t bos = -1, int32_t sep = -1, int32_t sepCount = 1, int32_t eos = -1, int32_t pad = 0, tkz_pair_truncation truncation = TKZ_PAIR_LONGEST_FIRST,
                              tkz_trim_side cutSide = TKZ_TRIM_SUFFIX, tkz_pad_side padSide = TKZ_PAD_RIGHT, int64_t padMultiple = 1) const {
        if (first.size() != second.size()) throw Error(TKZ_E_ARG, "EncodeBatchPairs: first and second must hold as many texts as each other");
        std::vector<uint16_t> units;
        std::vector<int64_t> offs{0};
        for (size_t i = 0; i < first.size(); ++i)
            for (const std::u16string* t : {&first[i], &second[i]}) { units.insert(units.end(), t->begin(), t->end()); offs.push_back(static_cast<int64_t>(units.size())); }
        return pairs_batch<uint16_t>(units, offs, maxLength, allowedSpecial, bos, sep, sepCount, eos, pad, truncation, cutSide, padSide, padMultiple, true);
    }
    // (the id of a registered special token, for bos / eos)
    int32_t SpecialTokenId(const std::string& literal) const {
        for (const auto& kv : specials_) if (kv.first == literal) return kv.second;
        throw Error(TKZ_E_ARG, "not a registered special token: " + literal);
    }
    // (one string: tkz_encode_trim_utf16, the single-text trim entry)
    Trimmed16 EncodeTrimSuffixUtf16(const std::u16string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        Trimmed16 out;
        return trim_one_device16(text, allowedSpecial, maxTokenCount, TKZ_TRIM_SUFFIX, out) ? out : trim_suffix_host16(text, allowedSpecial, maxTokenCount);
    }
    Trimmed16 EncodeTrimPrefixUtf16(const std::u16string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        Trimmed16 out;
        return trim_one_device16(text, allowedSpecial, maxTokenCount, TKZ_TRIM_PREFIX, out) ? out : trim_prefix_host16(text, allowedSpecial, maxTokenCount);
    }
    std::vector<Trimmed16> EncodeTrimSuffixBatchUtf16(const std::vector<std::u16string>& texts, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        std::vector<Trimmed16> out;
        if (trim_batch_device16(texts, allowedSpecial, maxTokenCount, TKZ_TRIM_SUFFIX, out)) return out;
        for (const std::u16string& t : texts) out.push_back(trim_suffix_host16(t, allowedSpecial, maxTokenCount));
        return out;
    }
    std::vector<Trimmed16> EncodeTrimPrefixBatchUtf16(const std::vector<std::u16string>& texts, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        std::vector<Trimmed16> out;
        if (trim_batch_device16(texts, allowedSpecial, maxTokenCount, TKZ_TRIM_PREFIX, out)) return out;
        for (const std::u16string& t : texts) out.push_back(trim_prefix_host16(t, allowedSpecial, maxTokenCount));
        return out;
    }
    // the host walk (the reference's loops over the string's code units): Encode, EncodeTrimSuffix, EncodeTrimPrefix
    std::vector<int32_t> encode_host16(const std::u16string& text, const std::vector<std::string>& allowedSpecial) const {
        std::vector<int32_t> ids;
        for (const PieceItem& it : piece_items16(text, allowedSpecial)) ids.insert(ids.end(), it.ids.begin(), it.ids.end());
        return ids;
    }
    Trimmed16 trim_suffix_host16(const std::u16string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        std::vector<int32_t> ids;
        int64_t tokenCount = 0; size_t encodeLength = 0;
        for (const PieceItem& it : piece_items16(text, allowedSpecial)) {
            tokenCount += static_cast<int64_t>(it.ids.size());
            if (tokenCount > maxTokenCount) break;
            ids.insert(ids.end(), it.ids.begin(), it.ids.end());
            encodeLength = it.end;
            if (tokenCount >= maxTokenCount) break;
        }
        return {ids, text.substr(0, encodeLength)};
    }
    Trimmed16 trim_prefix_host16(const std::u16string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount) const {
        std::vector<int32_t> ids;
        std::vector<std::pair<int64_t, size_t>> boundaries{{0, 0}};
        int64_t tokenCount = 0;
        for (const PieceItem& it : piece_items16(text, allowedSpecial)) {
            tokenCount += static_cast<int64_t>(it.ids.size());
            ids.insert(ids.end(), it.ids.begin(), it.ids.end());
            boundaries.push_back({tokenCount, it.end});
        }
        if (tokenCount <= maxTokenCount) return {ids, text};
        const int64_t prefix = tokenCount - maxTokenCount;
        int64_t cutTokens = 0; size_t cutLen = 0;
        for (const auto& b : boundaries) if (b.first >= prefix) { cutTokens = b.first; cutLen = b.second; break; }
        return {std::vector<int32_t>(ids.begin() + cutTokens, ids.end()), text.substr(cutLen)};
    }
    tkz_encoder* native() const { return enc_; }
    // the device workspace of batches of up to max_bytes / max_docs, allocated now instead of inside the first batch call (tkz_encoder_reserve): what
    // TokenizerBuilder.CreateTokenizer (TokenizerBuilder.cs:210-213) is for a drop-in -- construction pays, not the first Encode
    // ---- Decode (ITokenizer.cs:45, TikTokenizer.cs:586-604) ----
    // Decode / DecodeBatch: the bytes the reference hands to Encoding.UTF8.GetString (tkz_decode_batch) -- a std::string holds them as they are, well-formed or
    // not.  DecodeUtf16 / DecodeBatchUtf16: the string GetString makes of them, its code units from the device (tkz_decode_batch_utf16: one U+FFFD per maximal
    // subpart of an ill-formed sequence).  Ids that are neither in the vocabulary nor registered special tokens contribute nothing.
    std::vector<std::string> DecodeBatch(const std::vector<std::vector<int32_t>>& batches) const {
        return decode_batch<std::string, uint8_t>(batches, 8, tkz_decode_batch);
    }
    // (ONE id list: tkz_decode_utf8 / _utf16, a single kernel launch for up to 32,768 ids)
    std::string Decode(const std::vector<int32_t>& ids) const { return decode_one<std::string, uint8_t>(ids, 8, tkz_decode_utf8); }
    std::vector<std::u16string> DecodeBatchUtf16(const std::vector<std::vector<int32_t>>& batches) const {
        return decode_batch<std::u16string, uint16_t>(batches, 8, tkz_decode_batch_utf16);
    }
    std::u16string DecodeUtf16(const std::vector<int32_t>& ids) const { return decode_one<std::u16string, uint16_t>(ids, 8, tkz_decode_utf16); }
    void Reserve(int64_t max_bytes, int64_t max_docs) { check(tkz_encoder_reserve(enc_, max_bytes, max_docs)); }
    // The split is whatever the HOST's regex engine makes of the pattern (TikTokenizer.cs:77 compiles it in the running process).  A host on another
    // runtime than net6.0 hands its Unicode classification over (classes[cp] in 0..8 for cp < n: 65536 code units or 1114112 code points; nullptr:
    // the built-in Unicode 13.0 table) and says how it reads cl100k's (?i:...): .NET >= 7 folds U+017F onto `s`.
    void SetUnicodeClasses(const uint8_t* classes, int64_t n_code_points) { check(tkz_encoder_set_unicode_classes(enc_, classes, n_code_points)); }
    void SetCaseEquivalence(bool dotnet7_or_later) { check(tkz_encoder_set_option(enc_, TKZ_OPT_CASE_EQUIVALENCE, dotnet7_or_later ? 1 : 0)); }

private:
    struct Segment { bool special; int32_t id; size_t begin, end; };          // bytes [begin, end) of the text
    // one call of a decode entry on the ids of all batches (a second one when the first guess of the capacity, `per_id` elements an id, was too small)
    template <class Str, class Elem, class Entry>
    std::vector<Str> decode_batch(const std::vector<std::vector<int32_t>>& batches, size_t per_id, Entry entry) const {
        std::vector<int32_t> ids;
        std::vector<int64_t> offs{0};
        for (const auto& b : batches) { ids.insert(ids.end(), b.begin(), b.end()); offs.push_back(static_cast<int64_t>(ids.size())); }
        std::vector<Elem> out(ids.size() * per_id + 16);
        std::vector<int64_t> ooff(batches.size() + 1, 0);
        int64_t needed = 0;
        tkz_status st = entry(enc_, ids.data(), offs.data(), static_cast<int64_t>(batches.size()), out.data(), static_cast<int64_t>(out.size()), ooff.data(), &needed);
        if (st == TKZ_E_CAPACITY) {
            out.resize(static_cast<size_t>(needed));
            st = entry(enc_, ids.data(), offs.data(), static_cast<int64_t>(batches.size()), out.data(), static_cast<int64_t>(out.size()), ooff.data(), &needed);
        }
        check(st);
        std::vector<Str> res(batches.size());
        for (size_t d = 0; d < batches.size(); ++d)
            res[d].assign(reinterpret_cast<const typename Str::value_type*>(out.data()) + ooff[d], static_cast<size_t>(ooff[d + 1] - ooff[d]));
        return res;
    }
    template <class Str, class Elem, class Entry>
    Str decode_one(const std::vector<int32_t>& ids, size_t per_id, Entry entry) const {
        std::vector<Elem> out(ids.size() * per_id + 16);
        int64_t n = 0;
        tkz_status st = entry(enc_, ids.data(), static_cast<int64_t>(ids.size()), out.data(), static_cast<int64_t>(out.size()), &n);
        if (st == TKZ_E_CAPACITY) {
            out.resize(static_cast<size_t>(n));
            st = entry(enc_, ids.data(), static_cast<int64_t>(ids.size()), out.data(), static_cast<int64_t>(out.size()), &n);
        }
        check(st);
        return Str(reinterpret_cast<const typename Str::value_type*>(out.data()), static_cast<size_t>(n));
    }
    // EncodeInternal + FindNextSpecialToken (TikTokenizer.cs:141-170,230-241): plain segments and special literals in order
    std::vector<Segment> segments(const std::string& text, const std::vector<std::string>& allowedSpecial) const {
        std::vector<Segment> out;
        size_t start = 0;
        for (;;) {
            size_t hit_pos = std::string::npos; int hit = -1;
            if (!allowedSpecial.empty()) {
                size_t find = start;
                for (;;) {
                    hit = -1;
                    size_t p = find;
                    for (; p < text.size(); ++p) { hit = match_at(text, p); if (hit >= 0) break; }
                    if (hit < 0) break;
                    bool ok = false;
                    for (const auto& a : allowedSpecial) if (a == specials_[hit].first) { ok = true; break; }
                    if (ok) { hit_pos = p; break; }
                    find = p + 1;                                       // startFind = nextSpecial.Index + 1 (one UTF-16 unit; literals are ASCII)
                    while (find < text.size() && (static_cast<uint8_t>(text[find]) & 0xC0) == 0x80) ++find;
                }
            }
            const size_t end = hit >= 0 ? hit_pos : text.size();
            if (end > start) out.push_back({false, 0, start, end});
            if (hit < 0) break;
            out.push_back({true, specials_[hit].second, hit_pos, hit_pos + specials_[hit].first.size()});   // EncodeSpecialToken (:215-220)
            start = hit_pos + specials_[hit].first.size();
            if (start >= text.size()) break;
        }
        return out;
    }
    std::vector<std::string> all_specials() const {
        std::vector<std::string> all;
        for (const auto& s : specials_) all.push_back(s.first);
        return all;
    }
    // Encode(text, allowedSpecial) through tkz_encode_special_utf8; false (nothing encoded): nothing to allow, or the entry refused the registered set
    bool encode_special_single(const std::string& text, const std::vector<std::string>& allowedSpecial, std::vector<int32_t>& ids) const {
        if (allowedSpecial.empty() || specials_.empty() || special_on_host_) return false;
        const std::vector<int32_t> index = allowed_index(allowedSpecial);
        ids.resize(text.size() + 1);
        int64_t n = 0;
        const tkz_status st = tkz_encode_special_utf8(enc_, reinterpret_cast<const uint8_t*>(text.data()), static_cast<int64_t>(text.size()), index.data(),
                                                      static_cast<int32_t>(index.size()), ids.data(), static_cast<int64_t>(ids.size()), &n);
        if (st == TKZ_E_UNSUPPORTED) { special_on_host_ = true; ids.clear(); return false; }
        check(st);
        ids.resize(static_cast<size_t>(n));
        return true;
    }
    // ONE call of the batch span entry on the concatenated texts (UNIT: uint8_t bytes, uint16_t code units), cut into a TokenSpans per text
    template <class UNIT>
    std::vector<TokenSpans> spans_batch(std::vector<UNIT>& items, const std::vector<int64_t>& offs, const std::vector<std::string>& allowedSpecial, bool utf16) const {
        const int64_t n = static_cast<int64_t>(offs.size()) - 1;
        std::vector<TokenSpans> out(static_cast<size_t>(n));
        if (n == 0) return out;
        const bool plain = allowedSpecial.empty() || specials_.empty();
        const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
        const int64_t cap = std::max<int64_t>(1, static_cast<int64_t>(items.size()) * (utf16 ? 3 : 1));      // (a token per byte; a unit is at most three bytes)
        if (items.empty()) items.push_back(0);
        std::vector<int32_t> ids(static_cast<size_t>(cap)), starts(static_cast<size_t>(cap));
        std::vector<int64_t> ooff(static_cast<size_t>(n) + 1, 0);
        int64_t needed = 0;
        tkz_status st;
        if (utf16) st = tkz_encode_batch_spans_utf16(enc_, reinterpret_cast<const uint16_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()),
                                                     ids.data(), cap, ooff.data(), starts.data(), &needed);
        else st = tkz_encode_batch_spans_utf8(enc_, reinterpret_cast<const uint8_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()),
                                              ids.data(), cap, ooff.data(), starts.data(), nullptr, &needed);
        check(st);
        for (int64_t d = 0; d < n; ++d) {
            out[static_cast<size_t>(d)].ids.assign(ids.begin() + ooff[d], ids.begin() + ooff[d + 1]);
            out[static_cast<size_t>(d)].starts.assign(starts.begin() + ooff[d], starts.begin() + ooff[d + 1]);
        }
        return out;
    }
    // ONE call of the batch packed entry on the concatenated texts (UNIT: uint8_t bytes, uint16_t code units), with the capacities that always suffice (tkz.h)
    template <class UNIT>
    PackedRows packed_batch(std::vector<UNIT>& items, const std::vector<int64_t>& offs, int64_t rowLen, const std::vector<std::string>& allowedSpecial, int32_t bos, int32_t eos,
                            int32_t pad, bool utf16) const {
        const int64_t n = static_cast<int64_t>(offs.size()) - 1;
        PackedRows out;
        out.row_len = rowLen;
        const bool plain = allowedSpecial.empty() || specials_.empty();
        const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
        const int64_t framing = (bos >= 0) + (eos >= 0), bound = static_cast<int64_t>(items.size()) * (utf16 ? 3 : 1) + framing * n;      // (a token per byte; a unit is at most three bytes)
        const int64_t rows = rowLen >= 1 ? (bound + rowLen - 1) / rowLen : 0, cap = rows * std::max<int64_t>(rowLen, 0), scap = n + rows;
        if (items.empty()) items.push_back(0);
        out.ids.resize(static_cast<size_t>(std::max<int64_t>(cap, 1)));
        out.pos.resize(out.ids.size());
        out.seg_starts.resize(static_cast<size_t>(scap) + 1);
        out.doc_offsets.assign(static_cast<size_t>(n) + 1, 0);
        int64_t needed = 0, nseg = 0;
        tkz_status st;
        if (utf16) st = tkz_encode_batch_packed_utf16(enc_, reinterpret_cast<const uint16_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()), bos, eos,
                                                      rowLen, pad, out.ids.data(), cap, out.doc_offsets.data(), out.pos.data(), out.seg_starts.data(), scap, &out.total_tokens, &needed, &nseg);
        else st = tkz_encode_batch_packed_utf8(enc_, reinterpret_cast<const uint8_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()), bos, eos,
                                               rowLen, pad, out.ids.data(), cap, out.doc_offsets.data(), out.pos.data(), out.seg_starts.data(), scap, &out.total_tokens, &needed, &nseg);
        check(st);
        out.n_rows = needed / rowLen;
        out.ids.resize(static_cast<size_t>(needed));
        out.pos.resize(static_cast<size_t>(needed));
        out.seg_starts.resize(static_cast<size_t>(nseg) + 1);
        return out;
    }
    // ONE call of the batch padded entry on the concatenated texts (UNIT: uint8_t bytes, uint16_t code units), with the capacity that always suffices (tkz.h): a row of
    // maxLength a text
    template <class UNIT>
    PaddedRows padded_batch(std::vector<UNIT>& items, const std::vector<int64_t>& offs, int64_t maxLength, const std::vector<std::string>& allowedSpecial, int32_t bos, int32_t eos,
                            int32_t pad, tkz_trim_side cutSide, tkz_pad_side padSide, int64_t padMultiple, bool utf16) const {
        const int64_t n = static_cast<int64_t>(offs.size()) - 1;
        PaddedRows out;
        const bool plain = allowedSpecial.empty() || specials_.empty();
        const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
        const int64_t cap = maxLength >= 1 && maxLength <= INT32_MAX ? n * maxLength : 0;      // (a maxLength out of range is refused by the library)
        if (items.empty()) items.push_back(0);
        out.ids.resize(static_cast<size_t>(std::max<int64_t>(cap, 1)));
        out.pos.resize(out.ids.size());
        out.mask.resize(out.ids.size());
        out.lens.resize(static_cast<size_t>(std::max<int64_t>(n, 1)));
        tkz_status st;
        if (utf16) st = tkz_encode_batch_padded_utf16(enc_, reinterpret_cast<const uint16_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()), bos, eos,
                                                      maxLength, cutSide, padSide, pad, padMultiple, out.ids.data(), cap, out.mask.data(), out.pos.data(), out.lens.data(), nullptr,
                                                      &out.total_tokens, &out.width, &out.n_cut);
        else st = tkz_encode_batch_padded_utf8(enc_, reinterpret_cast<const uint8_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()), bos, eos,
                                               maxLength, cutSide, padSide, pad, padMultiple, out.ids.data(), cap, out.mask.data(), out.pos.data(), out.lens.data(), nullptr,
                                               &out.total_tokens, &out.width, &out.n_cut);
        check(st);
        out.ids.resize(static_cast<size_t>(n * out.width));
        out.pos.resize(out.ids.size());
        out.mask.resize(out.ids.size());
        out.lens.resize(static_cast<size_t>(n));
        return out;
    }
    // ONE call of the batch bucketed entry on the concatenated texts, with the capacity that always suffices (tkz.h): a row of maxLength a text
    template <class UNIT>
    BucketedRows bucketed_batch(std::vector<UNIT>& items, const std::vector<int64_t>& offs, int64_t maxLength, int64_t bucketRows, tkz_bucket_order order,
                                const std::vector<std::string>& allowedSpecial, int32_t bos, int32_t eos, int32_t pad, tkz_trim_side cutSide, tkz_pad_side padSide,
                                int64_t padMultiple, bool utf16) const {
        const int64_t n = static_cast<int64_t>(offs.size()) - 1;
        BucketedRows out;
        out.bucket_rows = bucketRows;
        const bool plain = allowedSpecial.empty() || specials_.empty();
        const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
        const int64_t cap = maxLength >= 1 && maxLength <= INT32_MAX ? n * maxLength : 0;      // (a maxLength out of range is refused by the library)
        const int64_t nb = bucketRows >= 1 ? (n + bucketRows - 1) / bucketRows : 0;            // (... and so are bucketRows)
        if (items.empty()) items.push_back(0);
        out.ids.resize(static_cast<size_t>(std::max<int64_t>(cap, 1)));
        out.pos.resize(out.ids.size());
        out.mask.resize(out.ids.size());
        out.lens.resize(static_cast<size_t>(std::max<int64_t>(n, 1)));
        out.order.resize(out.lens.size());
        out.rank.resize(out.lens.size());
        out.bucket_offsets.resize(static_cast<size_t>(nb) + 1);
        out.bucket_widths.resize(static_cast<size_t>(std::max<int64_t>(nb, 1)));
        tkz_status st;
        if (utf16) st = tkz_encode_batch_bucketed_utf16(enc_, reinterpret_cast<const uint16_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()), bos,
                                                        eos, maxLength, cutSide, padSide, pad, padMultiple, bucketRows, order, out.ids.data(), cap, out.mask.data(), out.pos.data(),
                                                        out.lens.data(), nullptr, out.order.data(), out.rank.data(), out.bucket_offsets.data(), out.bucket_widths.data(),
                                                        &out.total_tokens, &out.total_positions, &out.n_cut);
        else st = tkz_encode_batch_bucketed_utf8(enc_, reinterpret_cast<const uint8_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()), bos, eos,
                                                 maxLength, cutSide, padSide, pad, padMultiple, bucketRows, order, out.ids.data(), cap, out.mask.data(), out.pos.data(),
                                                 out.lens.data(), nullptr, out.order.data(), out.rank.data(), out.bucket_offsets.data(), out.bucket_widths.data(),
                                                 &out.total_tokens, &out.total_positions, &out.n_cut);
        check(st);
        out.ids.resize(static_cast<size_t>(out.total_positions));
        out.pos.resize(out.ids.size());
        out.mask.resize(out.ids.size());
        out.lens.resize(static_cast<size_t>(n));
        out.order.resize(static_cast<size_t>(n));
        out.rank.resize(static_cast<size_t>(n));
        out.bucket_widths.resize(static_cast<size_t>(nb));
        return out;
    }
    // ONE call of the batch budgeted entry on the concatenated texts, with the capacities that always suffice (tkz.h): a row of maxLength and a bucket a text
    template <class UNIT>
    BudgetedRows budgeted_batch(std::vector<UNIT>& items, const std::vector<int64_t>& offs, int64_t maxLength, int64_t maxTokens, int64_t maxRows, tkz_bucket_order order,
                                const std::vector<std::string>& allowedSpecial, int32_t bos, int32_t eos, int32_t pad, tkz_trim_side cutSide, tkz_pad_side padSide,
                                int64_t padMultiple, bool utf16) const {
        const int64_t n = static_cast<int64_t>(offs.size()) - 1;
        BudgetedRows out;
        const bool plain = allowedSpecial.empty() || specials_.empty();
        const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
        const int64_t cap = maxLength >= 1 && maxLength <= INT32_MAX ? n * maxLength : 0;      // (a maxLength out of range is refused by the library)
        if (items.empty()) items.push_back(0);
        out.ids.resize(static_cast<size_t>(std::max<int64_t>(cap, 1)));
        out.pos.resize(out.ids.size());
        out.mask.resize(out.ids.size());
        out.lens.resize(static_cast<size_t>(std::max<int64_t>(n, 1)));
        out.order.resize(out.lens.size());
        out.rank.resize(out.lens.size());
        out.bucket_offsets.resize(static_cast<size_t>(n) + 1);
        out.bucket_rows.resize(static_cast<size_t>(n) + 1);
        out.bucket_widths.resize(static_cast<size_t>(std::max<int64_t>(n, 1)));
        tkz_status st;
        if (utf16) st = tkz_encode_batch_budgeted_utf16(enc_, reinterpret_cast<const uint16_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()), bos,
                                                        eos, maxLength, cutSide, padSide, pad, padMultiple, maxTokens, maxRows, order, out.ids.data(), cap, out.mask.data(),
                                                        out.pos.data(), out.lens.data(), nullptr, out.order.data(), out.rank.data(), out.bucket_offsets.data(),
                                                        out.bucket_rows.data(), out.bucket_widths.data(), n, &out.total_tokens, &out.total_positions, &out.n_cut, &out.n_buckets);
        else st = tkz_encode_batch_budgeted_utf8(enc_, reinterpret_cast<const uint8_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()), bos, eos,
                                                 maxLength, cutSide, padSide, pad, padMultiple, maxTokens, maxRows, order, out.ids.data(), cap, out.mask.data(), out.pos.data(),
                                                 out.lens.data(), nullptr, out.order.data(), out.rank.data(), out.bucket_offsets.data(), out.bucket_rows.data(),
                                                 out.bucket_widths.data(), n, &out.total_tokens, &out.total_positions, &out.n_cut, &out.n_buckets);
        check(st);
        out.ids.resize(static_cast<size_t>(out.total_positions));
        out.pos.resize(out.ids.size());
        out.mask.resize(out.ids.size());
        out.lens.resize(static_cast<size_t>(n));
        out.order.resize(static_cast<size_t>(n));
        out.rank.resize(static_cast<size_t>(n));
        out.bucket_offsets.resize(static_cast<size_t>(out.n_buckets) + 1);
        out.bucket_rows.resize(static_cast<size_t>(out.n_buckets) + 1);
        out.bucket_widths.resize(static_cast<size_t>(out.n_buckets));
        return out;
    }
    // ONE call of the batch pair entry on the interleaved texts (documents 2p and 2p + 1: the two texts of row p), with the capacity that always suffices (tkz.h): a row
    // of maxLength a pair
    template <class UNIT>
    PairRows pairs_batch(std::vector<UNIT>& items, const std::vector<int64_t>& offs, int64_t maxLength, const std::vector<std::string>& allowedSpecial, int32_t bos, int32_t sep,
                         int32_t sepCount, int32_t eos, int32_t pad, tkz_pair_truncation truncation, tkz_trim_side cutSide, tkz_pad_side padSide, int64_t padMultiple, bool utf16) const {
        const int64_t nd = static_cast<int64_t>(offs.size()) - 1, n = nd / 2;
        PairRows out;
        if (sep == -1) sepCount = 0;                                                           // (no separator id: no separator)
        const bool plain = allowedSpecial.empty() || specials_.empty();
        const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
        const int64_t cap = maxLength >= 1 && maxLength <= INT32_MAX ? n * maxLength : 0;      // (a maxLength out of range is refused by the library)
        if (items.empty()) items.push_back(0);
        out.ids.resize(static_cast<size_t>(std::max<int64_t>(cap, 1)));
        out.pos.resize(out.ids.size());
        out.mask.resize(out.ids.size());
        out.type_ids.resize(out.ids.size());
        out.lens.resize(static_cast<size_t>(std::max<int64_t>(n, 1)));
        out.kept.resize(static_cast<size_t>(std::max<int64_t>(nd, 1)));
        tkz_status st;
        if (utf16) st = tkz_encode_batch_pairs_utf16(enc_, reinterpret_cast<const uint16_t*>(items.data()), offs.data(), nd, index.data(), static_cast<int32_t>(index.size()), bos, sep,
                                                     sepCount, eos, maxLength, truncation, cutSide, padSide, pad, padMultiple, out.ids.data(), cap, out.mask.data(),
                                                     out.type_ids.data(), out.pos.data(), out.lens.data(), out.kept.data(), nullptr, &out.total_tokens, &out.width, &out.n_cut);
        else st = tkz_encode_batch_pairs_utf8(enc_, reinterpret_cast<const uint8_t*>(items.data()), offs.data(), nd, index.data(), static_cast<int32_t>(index.size()), bos, sep,
                                              sepCount, eos, maxLength, truncation, cutSide, padSide, pad, padMultiple, out.ids.data(), cap, out.mask.data(), out.type_ids.data(),
                                              out.pos.data(), out.lens.data(), out.kept.data(), nullptr, &out.total_tokens, &out.width, &out.n_cut);
        check(st);
        out.ids.resize(static_cast<size_t>(n * out.width));
        out.pos.resize(out.ids.size());
        out.mask.resize(out.ids.size());
        out.type_ids.resize(out.ids.size());
        out.lens.resize(static_cast<size_t>(n));
        out.kept.resize(static_cast<size_t>(nd));
        return out;
    }
    // ONE call of the batch chunk entry on the concatenated texts (UNIT: uint8_t bytes, uint16_t code units), cut into a list of (ids, text) per text
    template <class UNIT, class STR>
    std::vector<std::vector<std::pair<std::vector<int32_t>, STR>>> chunks_batch(std::vector<UNIT>& items, const std::vector<int64_t>& offs, const std::vector<STR>& texts,
                                                                              const std::vector<std::string>& allowedSpecial, int maxTokenCount, bool utf16) const {
        const int64_t n = static_cast<int64_t>(offs.size()) - 1;
        std::vector<std::vector<std::pair<std::vector<int32_t>, STR>>> out(static_cast<size_t>(n));
        if (n == 0 && maxTokenCount >= 1) return out;
        const bool plain = allowedSpecial.empty() || specials_.empty();
        const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
        const int64_t total = static_cast<int64_t>(items.size()) * (utf16 ? 3 : 1), mx = maxTokenCount;      // (a token per byte; a unit is at most three bytes)
        const int64_t cap = std::max<int64_t>(1, total);
        const int64_t ccap = std::max<int64_t>(1, std::min<int64_t>(total, n + 2 * total / std::max<int64_t>(mx, 1)));      // (tkz.h: the chunks that always suffice)
        if (items.empty()) items.push_back(0);
        std::vector<int32_t> ids(static_cast<size_t>(cap));
        std::vector<int64_t> ooff(static_cast<size_t>(n) + 1, 0), dco(static_cast<size_t>(n) + 1, 0), ct(static_cast<size_t>(ccap) + 1, 0), starts(static_cast<size_t>(ccap), 0);
        int64_t needed = 0, chunks = 0;
        tkz_status st;
        if (utf16) st = tkz_encode_batch_chunks_utf16(enc_, reinterpret_cast<const uint16_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()), mx,
                                                      ids.data(), cap, ooff.data(), dco.data(), ct.data(), starts.data(), ccap, &needed, &chunks);
        else st = tkz_encode_batch_chunks_utf8(enc_, reinterpret_cast<const uint8_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()), mx,
                                               ids.data(), cap, ooff.data(), dco.data(), ct.data(), starts.data(), nullptr, ccap, &needed, &chunks);
        check(st);
        for (int64_t d = 0; d < n; ++d) {
            const STR& t = texts[static_cast<size_t>(d)];
            for (int64_t c = dco[d]; c < dco[d + 1]; ++c) {
                const size_t a = static_cast<size_t>(starts[c]), b = c + 1 < dco[d + 1] ? static_cast<size_t>(starts[c + 1]) : t.size();
                out[static_cast<size_t>(d)].emplace_back(std::vector<int32_t>(ids.begin() + ct[c], ids.begin() + ct[c + 1]), t.substr(a, b - a));
            }
        }
        return out;
    }
    // chunks_batch for the overlap entries: every chunk has a start and an end, in tokens and in bytes (std::string) or code units (std::u16string)
    template <class UNIT, class STR>
    std::vector<std::vector<std::pair<std::vector<int32_t>, STR>>> chunks_overlap_batch(std::vector<UNIT>& items, const std::vector<int64_t>& offs, const std::vector<STR>& texts,
                                                                                      const std::vector<std::string>& allowedSpecial, int maxTokenCount, int overlap,
                                                                                      bool utf16) const {
        const int64_t n = static_cast<int64_t>(offs.size()) - 1;
        std::vector<std::vector<std::pair<std::vector<int32_t>, STR>>> out(static_cast<size_t>(n));
        if (n == 0 && maxTokenCount >= 1 && overlap >= 0 && overlap < maxTokenCount) return out;
        const bool plain = allowedSpecial.empty() || specials_.empty();
        const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
        const int64_t total = static_cast<int64_t>(items.size()) * (utf16 ? 3 : 1), mx = maxTokenCount, ov = overlap;
        const int64_t cap = std::max<int64_t>(1, total);
        const int64_t ccap = std::max<int64_t>(1, std::min<int64_t>(total, n + 2 * total / std::max<int64_t>(mx - ov, 1)));      // (tkz.h: the chunks that always suffice)
        if (items.empty()) items.push_back(0);
        std::vector<int32_t> ids(static_cast<size_t>(cap));
        std::vector<int64_t> ooff(static_cast<size_t>(n) + 1, 0), dco(static_cast<size_t>(n) + 1, 0);
        std::vector<int64_t> ct(static_cast<size_t>(ccap), 0), ce(static_cast<size_t>(ccap), 0), starts(static_cast<size_t>(ccap), 0), ends(static_cast<size_t>(ccap), 0);
        int64_t needed = 0, chunks = 0;
        tkz_status st;
        if (utf16) st = tkz_encode_batch_chunks_overlap_utf16(enc_, reinterpret_cast<const uint16_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()),
                                                              mx, ov, ids.data(), cap, ooff.data(), dco.data(), ct.data(), ce.data(), starts.data(), ends.data(), ccap, &needed,
                                                              &chunks);
        else st = tkz_encode_batch_chunks_overlap_utf8(enc_, reinterpret_cast<const uint8_t*>(items.data()), offs.data(), n, index.data(), static_cast<int32_t>(index.size()), mx,
                                                       ov, ids.data(), cap, ooff.data(), dco.data(), ct.data(), ce.data(), starts.data(), nullptr, ends.data(), nullptr, ccap,
                                                       &needed, &chunks);
        check(st);
        for (int64_t d = 0; d < n; ++d) {
            const STR& t = texts[static_cast<size_t>(d)];
            for (int64_t c = dco[d]; c < dco[d + 1]; ++c) {
                const size_t a = static_cast<size_t>(starts[c]), b = static_cast<size_t>(ends[c]);
                out[static_cast<size_t>(d)].emplace_back(std::vector<int32_t>(ids.begin() + ct[c], ids.begin() + ce[c]), t.substr(a, b - a));
            }
        }
        return out;
    }
    std::vector<int32_t> allowed_index(const std::vector<std::string>& allowedSpecial) const {
        std::vector<int32_t> index;
        for (size_t i = 0; i < specials_.size(); ++i)
            for (const auto& al : allowedSpecial) if (al == specials_[i].first) { index.push_back(static_cast<int32_t>(i)); break; }
        return index;
    }
    // well-formed UTF-8 -> UTF-16 (the registered literals), UTF-16 -> UTF-8 as Encoding.UTF8.GetBytes (a lone surrogate becomes EF BF BD)
    static std::u16string to_utf16(const std::string& s8) {
        std::u16string o;
        for (size_t i = 0; i < s8.size();) {
            const uint8_t c = static_cast<uint8_t>(s8[i]);
            const int len = c < 0x80 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4;
            uint32_t cp = len == 1 ? c : c & (0xFFu >> (len + 1));
            for (int k = 1; k < len && i + k < s8.size(); ++k) cp = (cp << 6) | (static_cast<uint8_t>(s8[i + k]) & 0x3Fu);
            if (cp >= 0x10000) { cp -= 0x10000; o.push_back(static_cast<char16_t>(0xD800 + (cp >> 10))); o.push_back(static_cast<char16_t>(0xDC00 + (cp & 0x3FF))); }
            else o.push_back(static_cast<char16_t>(cp));
            i += static_cast<size_t>(len);
        }
        return o;
    }
    static void append_utf8(const std::u16string& t, size_t begin, size_t end, std::vector<uint8_t>& o) {
        for (size_t i = begin; i < end; ++i) {
            uint32_t c = t[i];
            if (c >= 0xD800 && c <= 0xDBFF && i + 1 < end && t[i + 1] >= 0xDC00 && t[i + 1] <= 0xDFFF) { c = 0x10000 + ((c - 0xD800) << 10) + (t[i + 1] - 0xDC00); ++i; }
            else if (c >= 0xD800 && c <= 0xDFFF) c = 0xFFFD;
            if (c < 0x80) o.push_back(static_cast<uint8_t>(c));
            else if (c < 0x800) { o.push_back(static_cast<uint8_t>(0xC0 | (c >> 6))); o.push_back(static_cast<uint8_t>(0x80 | (c & 0x3F))); }
            else if (c < 0x10000) { o.push_back(static_cast<uint8_t>(0xE0 | (c >> 12))); o.push_back(static_cast<uint8_t>(0x80 | ((c >> 6) & 0x3F))); o.push_back(static_cast<uint8_t>(0x80 | (c & 0x3F))); }
            else { o.push_back(static_cast<uint8_t>(0xF0 | (c >> 18))); o.push_back(static_cast<uint8_t>(0x80 | ((c >> 12) & 0x3F))); o.push_back(static_cast<uint8_t>(0x80 | ((c >> 6) & 0x3F))); o.push_back(static_cast<uint8_t>(0x80 | (c & 0x3F))); }
        }
    }
    // EncodeInternal + FindNextSpecialToken on the code units: a literal matches where the string's units are the literal's
    std::vector<Segment> segments16(const std::u16string& text, const std::vector<std::string>& allowedSpecial) const {
        std::vector<std::u16string> lits;
        for (const auto& sp : specials_) lits.push_back(to_utf16(sp.first));
        auto match_at16 = [&](size_t p) { for (size_t i = 0; i < lits.size(); ++i) if (!lits[i].empty() && text.compare(p, lits[i].size(), lits[i]) == 0) return static_cast<int>(i); return -1; };
        std::vector<Segment> out;
        size_t start = 0;
        for (;;) {
            size_t hit_pos = std::u16string::npos; int hit = -1;
            if (!allowedSpecial.empty()) {
                for (size_t find = start;;) {
                    hit = -1;
                    size_t p = find;
                    for (; p < text.size(); ++p) { hit = match_at16(p); if (hit >= 0) break; }
                    if (hit < 0) break;
                    bool ok = false;
                    for (const auto& al : allowedSpecial) if (al == specials_[static_cast<size_t>(hit)].first) { ok = true; break; }
                    if (ok) { hit_pos = p; break; }
                    find = p + 1;                                       // startFind = nextSpecial.Index + 1
                }
            }
            const size_t end = hit >= 0 ? hit_pos : text.size();
            if (end > start) out.push_back({false, 0, start, end});
            if (hit < 0) break;
            out.push_back({true, specials_[static_cast<size_t>(hit)].second, hit_pos, hit_pos + lits[static_cast<size_t>(hit)].size()});
            start = hit_pos + lits[static_cast<size_t>(hit)].size();
            if (start >= text.size()) break;
        }
        return out;
    }
    // one item per regex piece of every plain segment and one per special token: its ids and the UNIT position where it ends (PieceItem below)
    bool trim_batch_device16(const std::vector<std::u16string>& texts, const std::vector<std::string>& allowedSpecial, int maxTokenCount, int32_t side, std::vector<Trimmed16>& out) const {
        const bool plain = allowedSpecial.empty() || specials_.empty();
        if (maxTokenCount < 0 || (!plain && special_on_host_)) return false;
        const int64_t n = static_cast<int64_t>(texts.size());
        if (n == 0) return true;
        const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
        std::vector<uint16_t> units;
        std::vector<int64_t> offs{0};
        for (const std::u16string& t : texts) { units.insert(units.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(units.size())); }
        const int64_t total = offs[static_cast<size_t>(n)];
        const int64_t cap = std::min<int64_t>(3 * total, n * static_cast<int64_t>(maxTokenCount));
        std::vector<int32_t> ids(static_cast<size_t>(cap) + 1);
        std::vector<int64_t> ooff(static_cast<size_t>(n) + 1, 0), cut(static_cast<size_t>(n), 0);
        int64_t needed = 0;
        if (units.empty()) units.push_back(0);
        const tkz_status st = tkz_encode_batch_trim_utf16(enc_, units.data(), offs.data(), n, index.empty() ? nullptr : index.data(), static_cast<int32_t>(index.size()), side,
                                                          maxTokenCount, nullptr, ids.data(), cap, ooff.data(), cut.data(), &needed);
        if (st == TKZ_E_UNSUPPORTED) { special_on_host_ = true; return false; }
        check(st);
        for (size_t t = 0; t < texts.size(); ++t) {
            const size_t c = static_cast<size_t>(cut[t]);             // code units of the kept text (suffix) / of the dropped text (prefix)
            out.push_back({std::vector<int32_t>(ids.begin() + ooff[t], ids.begin() + ooff[t + 1]), side == TKZ_TRIM_SUFFIX ? texts[t].substr(0, c) : texts[t].substr(c)});
        }
        return true;
    }
    // ONE text on the single-text trim entries; false (nothing done): the host walk has to do it -- the cases of trim_batch_device
    bool trim_one_device(const std::string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount, int32_t side, Trimmed& out) const {
        const bool plain = allowedSpecial.empty() || specials_.empty();
        if (maxTokenCount < 0 || (!plain && special_on_host_)) return false;
        const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
        const int64_t cap = std::min<int64_t>(static_cast<int64_t>(text.size()), maxTokenCount);
        std::vector<int32_t> ids(static_cast<size_t>(cap) + 1);
        int64_t n = 0, cut = 0;
        const tkz_status st = tkz_encode_trim_utf8(enc_, reinterpret_cast<const uint8_t*>(text.data()), static_cast<int64_t>(text.size()), index.empty() ? nullptr : index.data(),
                                                   static_cast<int32_t>(index.size()), side, maxTokenCount, ids.data(), cap, &n, &cut, nullptr);
        if (st == TKZ_E_UNSUPPORTED) { special_on_host_ = true; return false; }
        check(st);
        ids.resize(static_cast<size_t>(n));
        const size_t c = static_cast<size_t>(cut);                    // bytes of the kept text (suffix) / of the dropped text (prefix)
        out = {ids, side == TKZ_TRIM_SUFFIX ? text.substr(0, c) : text.substr(c)};
        return true;
    }
    bool trim_one_device16(const std::u16string& text, const std::vector<std::string>& allowedSpecial, int maxTokenCount, int32_t side, Trimmed16& out) const {
        const bool plain = allowedSpecial.empty() || specials_.empty();
        if (maxTokenCount < 0 || (!plain && special_on_host_)) return false;
        const std::vector<int32_t> index = plain ? std::vector<int32_t>{} : allowed_index(allowedSpecial);
        const int64_t cap = std::min<int64_t>(3 * static_cast<int64_t>(text.size()), maxTokenCount);
        std::vector<int32_t> ids(static_cast<size_t>(cap) + 1);
        int64_t n = 0, cut = 0;
        const tkz_status st = tkz_encode_trim_utf16(enc_, reinterpret_cast<const uint16_t*>(text.data()), static_cast<int64_t>(text.size()), index.empty() ? nullptr : index.data(),
                                                    static_cast<int32_t>(index.size()), side, maxTokenCount, ids.data(), cap, &n, &cut);
        if (st == TKZ_E_UNSUPPORTED) { special_on_host_ = true; return false; }
        check(st);
        ids.resize(static_cast<size_t>(n));
        const size_t c = static_cast<size_t>(cut);                    // code units of the kept text (suffix) / of the dropped text (prefix)
        out = {ids, side == TKZ_TRIM_SUFFIX ? text.substr(0, c) : text.substr(c)};
        return true;
    }
    // the batch on the device's trim entry; false (nothing done): the host walk has to do it
    bool trim_batch_device(const std::vector<std::string>& texts, const std::vector<std::string>& allowedSpecial, int maxTokenCount, int32_t side, std::vector<Trimmed>& out) const {
        const bool plain = allowedSpecial.empty() || specials_.empty();
        if (maxTokenCount < 0 || (!plain && special_on_host_)) return false;
        const int64_t n = static_cast<int64_t>(texts.size());
        if (n == 0) return true;
        std::vector<int32_t> index;
        if (!plain)
            for (size_t i = 0; i < specials_.size(); ++i)
                for (const auto& a : allowedSpecial) if (a == specials_[i].first) { index.push_back(static_cast<int32_t>(i)); break; }
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (const std::string& t : texts) { bytes.insert(bytes.end(), t.begin(), t.end()); offs.push_back(static_cast<int64_t>(bytes.size())); }
        const int64_t total = offs[static_cast<size_t>(n)];
        const int64_t cap = std::min<int64_t>(total, n * static_cast<int64_t>(maxTokenCount));       // (tkz.h: always sufficient)
        std::vector<int32_t> ids(static_cast<size_t>(cap) + 1);
        std::vector<int64_t> ooff(static_cast<size_t>(n) + 1, 0), cut(static_cast<size_t>(n), 0);
        int64_t needed = 0;
        if (bytes.empty()) bytes.push_back(0);
        const tkz_status st = tkz_encode_batch_trim_utf8(enc_, bytes.data(), offs.data(), n, index.empty() ? nullptr : index.data(), static_cast<int32_t>(index.size()), side,
                                                         maxTokenCount, nullptr, ids.data(), cap, ooff.data(), cut.data(), nullptr, &needed);
        if (st == TKZ_E_UNSUPPORTED) { special_on_host_ = true; return false; }
        check(st);
        for (size_t t = 0; t < texts.size(); ++t) {
            const size_t c = static_cast<size_t>(cut[t]);             // bytes of the kept text (suffix) / of the dropped text (prefix)
            out.push_back({std::vector<int32_t>(ids.begin() + ooff[t], ids.begin() + ooff[t + 1]), side == TKZ_TRIM_SUFFIX ? texts[t].substr(0, c) : texts[t].substr(c)});
        }
        return true;
    }
    // one item per regex piece of every plain segment and one per special token: its ids and the byte position where it ends
    struct PieceItem { std::vector<int32_t> ids; size_t end; };
    std::vector<PieceItem> piece_items(const std::string& text, const std::vector<std::string>& allowedSpecial) const {
        const std::vector<Segment> segs = segments(text, allowedSpecial);
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (const Segment& g : segs)
            if (!g.special) { bytes.insert(bytes.end(), text.begin() + g.begin, text.begin() + g.end); offs.push_back(static_cast<int64_t>(bytes.size())); }
        const int64_t nseg = static_cast<int64_t>(offs.size()) - 1;
        const size_t cap = bytes.size() ? bytes.size() : 1;
        std::vector<int32_t> ids(cap);
        std::vector<int64_t> dpo(static_cast<size_t>(nseg) + 1, 0), pbo(cap + 1, 0), pto(cap + 1, 0);
        int64_t npieces = 0, needed = 0;
        if (bytes.empty()) bytes.push_back(0);
        check(tkz_encode_batch_pieces_utf8(enc_, bytes.data(), offs.data(), nseg, ids.data(), static_cast<int64_t>(cap), dpo.data(), pbo.data(),
                                           pto.data(), static_cast<int64_t>(cap), &npieces, &needed));
        std::vector<PieceItem> out;
        int64_t k = 0;
        for (const Segment& g : segs) {
            if (g.special) { out.push_back({{g.id}, g.end}); continue; }
            for (int64_t p = dpo[k]; p < dpo[k + 1]; ++p)
                out.push_back({std::vector<int32_t>(ids.begin() + pto[p], ids.begin() + pto[p + 1]),
                               g.begin + static_cast<size_t>(pbo[p + 1] - offs[k])});
            ++k;
        }
        return out;
    }
    // the same over code units: every plain segment is transcoded here as GetBytes does, its pieces come from the piece-granular entry, and a piece's end
    // goes back to units (one per non-continuation byte, one more per 4-byte char)
    std::vector<PieceItem> piece_items16(const std::u16string& text, const std::vector<std::string>& allowedSpecial) const {
        const std::vector<Segment> segs = segments16(text, allowedSpecial);
        std::vector<uint8_t> bytes;
        std::vector<int64_t> offs{0};
        for (const Segment& g : segs)
            if (!g.special) { append_utf8(text, g.begin, g.end, bytes); offs.push_back(static_cast<int64_t>(bytes.size())); }
        const int64_t nseg = static_cast<int64_t>(offs.size()) - 1;
        const size_t cap = bytes.size() ? bytes.size() : 1;
        std::vector<int32_t> ids(cap);
        std::vector<int64_t> dpo(static_cast<size_t>(nseg) + 1, 0), pbo(cap + 1, 0), pto(cap + 1, 0);
        int64_t npieces = 0, needed = 0;
        if (bytes.empty()) bytes.push_back(0);
        check(tkz_encode_batch_pieces_utf8(enc_, bytes.data(), offs.data(), nseg, ids.data(), static_cast<int64_t>(cap), dpo.data(), pbo.data(),
                                           pto.data(), static_cast<int64_t>(cap), &npieces, &needed));
        std::vector<PieceItem> out;
        int64_t k = 0;
        for (const Segment& g : segs) {
            if (g.special) { out.push_back({{g.id}, g.end}); continue; }
            size_t unit = g.begin;
            int64_t b = offs[k];
            for (int64_t p = dpo[k]; p < dpo[k + 1]; ++p) {
                for (; b < pbo[p + 1]; ++b) unit += ((bytes[static_cast<size_t>(b)] & 0xC0) != 0x80 ? 1u : 0u) + (bytes[static_cast<size_t>(b)] >= 0xF0 ? 1u : 0u);
                out.push_back({std::vector<int32_t>(ids.begin() + pto[p], ids.begin() + pto[p + 1]), unit});
            }
            ++k;
        }
        return out;
    }
    // The work of EncodeBatchFlat on nseg segments, seg_at(i) = (pointer, length) of segment i: the ids land in out.out_ids_, the offsets
    // (nseg + 1) in out.out_offs_.  Everything that touches every segment runs on `threads` host threads (0: one per ~16 k segments, at most
    // 16): the segment offsets (a two-pass prefix sum) and the gather into page-locked memory.  The gather is cut into sub-batches of ~128 MB
    // and runs AHEAD of the device: the workers go through the sub-batches in order without waiting for anything, the calling thread hands
    // sub-batch k to tkz_encode_batch_utf8 (which overlaps upload, kernels and download among its own chunks) as soon as it is gathered.
    // A token is at least one byte, English-like text has one per ~4: room for a token per two bytes first; when that was not enough, room
    // for a token per byte (always enough) and the calls again.
    struct Joiner { std::vector<std::thread> pool; ~Joiner() { for (std::thread& t : pool) if (t.joinable()) t.join(); } };
    // allowed: null, or the indices of the allowed special tokens -- the segments are then whole texts and go to tkz_encode_batch_special_utf8; returns false
    // (nothing encoded) when that entry refuses the registered set with TKZ_E_UNSUPPORTED, true otherwise.
    template <class SegAt>
    bool encode_segments(int64_t nseg, SegAt seg_at, FlatBatch& out, int threads, const std::vector<int32_t>* allowed = nullptr) const {
        int nth = threads > 0 ? threads : static_cast<int>(std::min<int64_t>(16, nseg >> 14));
        const unsigned hw = std::thread::hardware_concurrency();
        if (hw && nth > static_cast<int>(hw)) nth = static_cast<int>(hw);
        if (nth < 1) nth = 1;
        const auto t_begin = std::chrono::steady_clock::now();
        auto ms_since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
        int64_t* offs = static_cast<int64_t*>(out.in_offs_.ensure((static_cast<size_t>(nseg) + 1) * 8));
        auto slice = [&](int t) { return nseg * t / nth; };      // thread t owns segments [slice(t), slice(t + 1)) of every pass over the segments
        // 1. offsets: every thread sums its slice, then writes its offsets from the sum of the slices before it
        offs[0] = 0;
        if (nth == 1) { for (int64_t i = 0; i < nseg; ++i) offs[i + 1] = offs[i] + static_cast<int64_t>(seg_at(i).second); }
        else {
            std::vector<int64_t> part(static_cast<size_t>(nth) + 1, 0);
            { Joiner j; for (int t = 0; t < nth; ++t) j.pool.emplace_back([&, t] { int64_t sum = 0; for (int64_t i = slice(t); i < slice(t + 1); ++i) sum += static_cast<int64_t>(seg_at(i).second); part[static_cast<size_t>(t) + 1] = sum; }); }
            for (int t = 0; t < nth; ++t) part[static_cast<size_t>(t) + 1] += part[static_cast<size_t>(t)];
            { Joiner j; for (int t = 0; t < nth; ++t) j.pool.emplace_back([&, t] { int64_t at = part[static_cast<size_t>(t)]; for (int64_t i = slice(t); i < slice(t + 1); ++i) { at += static_cast<int64_t>(seg_at(i).second); offs[i + 1] = at; } }); }
        }
        const int64_t total = offs[nseg];
        out.last_offsets_ms = ms_since(t_begin); out.last_wait_ms = out.last_encode_ms = 0;
        uint8_t* bytes = static_cast<uint8_t*>(out.in_bytes_.ensure(static_cast<size_t>(total) + 64));
        // 2. sub-batches
        static const int64_t kSubBytes = [] { const char* v = std::getenv("TKZ_FLAT_SUBBATCH_BYTES"); const long long n = v ? std::atoll(v) : 0; return n > 0 ? static_cast<int64_t>(n) : (int64_t(128) << 20); }();
        const int nsb = total >= 2 * kSubBytes ? static_cast<int>(std::min<int64_t>(64, total / kSubBytes)) : 1;
        std::vector<int64_t> cut(static_cast<size_t>(nsb) + 1, 0);
        cut[static_cast<size_t>(nsb)] = nseg;
        for (int k = 1; k < nsb; ++k) cut[static_cast<size_t>(k)] = std::lower_bound(offs, offs + nseg, total / nsb * k) - offs;
        // the offsets of sub-batch k, starting at 0 as the entry point wants them: sub[cut[k] + k .. cut[k + 1] + k]
        int64_t* sub = nsb > 1 ? static_cast<int64_t*>(out.sub_offs_.ensure((static_cast<size_t>(nseg) + static_cast<size_t>(nsb) + 1) * 8)) : offs;
        std::vector<std::atomic<int>> done(static_cast<size_t>(nsb));
        for (auto& d : done) d.store(0, std::memory_order_relaxed);
        auto gather_slice = [&](int k, int t) {                  // thread t's share of sub-batch k: about the same number of bytes for every thread
            const int64_t lo0 = cut[static_cast<size_t>(k)], hi0 = cut[static_cast<size_t>(k) + 1], b0 = offs[lo0], nb = offs[hi0] - b0;
            const int64_t lo = t == 0 ? lo0 : std::lower_bound(offs + lo0, offs + hi0, b0 + nb / nth * t) - offs;
            const int64_t hi = t == nth - 1 ? hi0 : std::lower_bound(offs + lo0, offs + hi0, b0 + nb / nth * (t + 1)) - offs;
            for (int64_t i = lo; i < hi; ++i) {
                const std::pair<const char*, size_t> g = seg_at(i);
                std::memcpy(bytes + offs[i], g.first, g.second);
                if (nsb > 1) sub[i + k] = offs[i] - b0;
            }
            if (nsb > 1 && t == nth - 1) sub[hi0 + k] = nb;
        };
        Joiner workers;
        if (nth == 1 && nsb == 1) { gather_slice(0, 0); done[0].store(1, std::memory_order_release); }
        else for (int t = 0; t < nth; ++t)
            workers.pool.emplace_back([&, t] { for (int k = 0; k < nsb; ++k) { gather_slice(k, t); done[static_cast<size_t>(k)].fetch_add(1, std::memory_order_release); } });
        const int need = (nth == 1 && nsb == 1) ? 1 : nth;
        // 3. encode
        int64_t* ooff = static_cast<int64_t*>(out.out_offs_.ensure((static_cast<size_t>(nseg) + 1) * 8));
        bool full = false;
        for (int attempt = 0;; ++attempt) {
            const int64_t cap = full ? std::max<int64_t>(1, total)
                                     : std::max<int64_t>(1, std::min<int64_t>(total, std::max<int64_t>(total / 2 + 4096, static_cast<int64_t>(static_cast<double>(total) * out.tokens_per_byte_ * 1.1))));
            int32_t* ids = static_cast<int32_t*>(out.out_ids_.ensure(static_cast<size_t>(cap) * 4));
            int64_t tok_base = 0;
            bool over = false;
            for (int k = 0; k < nsb && !over; ++k) {
                const auto t_w = std::chrono::steady_clock::now();
                while (done[static_cast<size_t>(k)].load(std::memory_order_acquire) < need) std::this_thread::yield();
                out.last_wait_ms += ms_since(t_w);
                const auto t_e = std::chrono::steady_clock::now();
                const int64_t d0 = cut[static_cast<size_t>(k)], nd = cut[static_cast<size_t>(k) + 1] - d0;
                int64_t needed = 0;
                const tkz_status st = allowed ? tkz_encode_batch_special_utf8(enc_, bytes + offs[d0], nsb > 1 ? sub + d0 + k : offs, nd, allowed->data(), static_cast<int32_t>(allowed->size()),
                                                                              ids + tok_base, cap - tok_base, ooff + d0, &needed)
                                              : tkz_encode_batch_utf8(enc_, bytes + offs[d0], nsb > 1 ? sub + d0 + k : offs, nd, ids + tok_base, cap - tok_base, ooff + d0, &needed);
                out.last_encode_ms += ms_since(t_e);
                if (allowed && st == TKZ_E_UNSUPPORTED) return false;        // (the first sub-batch says so: the literal set is the encoder's)
                if (st == TKZ_E_CAPACITY) { over = true; break; }
                check(st);
                if (tok_base) for (int64_t i = d0; i <= d0 + nd; ++i) ooff[i] += tok_base;
                tok_base += needed;
            }
            if (!over) break;
            if (attempt || cap >= total) check(TKZ_E_CAPACITY);                      // (cannot happen: a token per byte is always enough)
            full = true;
        }
        if (total > 0) out.tokens_per_byte_ = std::max(out.tokens_per_byte_, static_cast<double>(ooff[nseg]) / static_cast<double>(total));
        return true;
    }
    int match_at(const std::string& text, size_t p) const {       // first registered literal that matches at p
        for (size_t i = 0; i < specials_.size(); ++i) {
            const std::string& lit = specials_[i].first;
            if (!lit.empty() && text.compare(p, lit.size(), lit) == 0) return static_cast<int>(i);
        }
        return -1;
    }
    SpecialTokens specials_;
    mutable bool special_on_host_ = false;     // the device's special entries refused the registered set: EncodeBatchFlat segments on the host
    tkz_encoder* enc_ = nullptr;
};

struct TokenizerBuilder {
    // TokenizerBuilder.CreateTokenizer(Stream, IReadOnlyDictionary<string,int>, string pattern, int cacheSize)
    static TikTokenizer* CreateTokenizer(const std::string& tikTokenBpeFile, SpecialTokens specialTokensEncoder, const std::string& pattern,
                                         int cacheSize = 8192, int device = 0) {
        TikTokenizer* t = new TikTokenizer(tikTokenBpeFile, std::move(specialTokensEncoder), pattern, device);
        // the reference's LRU piece memo (LRUCache.cs; no effect on results) lives on the device with a fixed size: cacheSize says whether it is used
        if (cacheSize <= 0) (void)tkz_encoder_set_option(t->native(), TKZ_OPT_PIECE_MEMO, 0);
        return t;
    }
};

}  // namespace tkz
