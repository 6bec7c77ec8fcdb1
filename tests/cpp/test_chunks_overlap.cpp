// The overlap chunk methods of the C++ host mirror (include/tkz_tokenizer.hpp) -- EncodeChunksOverlap, EncodeChunksOverlapBatch and their Utf16 forms --, which
// call tkz_encode_batch_chunks_overlap_utf8 / _utf16: every chunk's text against the keys Decode returns for its ids, the chunks against the caller's own loop
// over EncodeTrimSuffix and EncodeTrimPrefix (while no piece exceeds the budget), overlap 0 against EncodeChunks, the first and the last chunk against the
// ends of the text and of Encode's ids, with the calls read from tkz_encoder_chunks_overlap_calls.  Built by tests/test_cpp_chunks_overlap.py against the emulated library on CPU and
// against libtkz.so on the GPU.  argv: gpt2.tiktoken
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using Chunks = std::vector<tkz::TikTokenizer::Trimmed>;
static int64_t calls(const tkz::TikTokenizer& tok) { int64_t c = 0; tkz_encoder_chunks_overlap_calls(tok.native(), &c); return c; }
static std::u16string widen(const std::string& ascii) { return std::u16string(ascii.begin(), ascii.end()); }

// every text is the keys of its ids, no chunk is empty or over the budget, the first chunk starts the text and Encode's ids, the last ends them.  (Where a
// chunk starts among repeated ids cannot be told from (ids, text) alone: the caller's loop below and overlap 0 against EncodeChunks pin that.)
static bool well_formed(const tkz::TikTokenizer& tok, const std::string& text, const std::vector<int32_t>& ids, const Chunks& ch, int mx) {
    if (ch.empty()) return text.empty() && ids.empty();
    for (const auto& c : ch)
        if (c.first.empty() || c.first.size() > static_cast<size_t>(mx) || tok.Decode(c.first) != c.second) return false;
    const auto& f = ch.front();
    const auto& l = ch.back();
    if (f.first.size() > ids.size() || l.first.size() > ids.size() || l.second.size() > text.size()) return false;
    return std::equal(f.first.begin(), f.first.end(), ids.begin()) && text.compare(0, f.second.size(), f.second) == 0 &&
           std::equal(l.first.begin(), l.first.end(), ids.end() - static_cast<std::ptrdiff_t>(l.first.size())) &&
           text.compare(text.size() - l.second.size(), l.second.size(), l.second) == 0;
}
// the caller's loop over the two trim functions; false when it would spin (the next piece alone exceeds the budget)
static bool trim_loop(const tkz::TikTokenizer& tok, const std::string& text, const std::vector<std::string>& allowed, int mx, int ov, Chunks& out) {
    size_t p = 0;
    while (p < text.size()) {
        const std::string rest = text.substr(p);
        tkz::TikTokenizer::Trimmed t = tok.EncodeTrimSuffix(rest, allowed, mx);
        if (t.first.empty()) return false;
        const std::string part = t.second;
        const size_t n_ids = t.first.size();
        out.push_back(std::move(t));
        if (part.size() == rest.size()) break;
        size_t next = p + part.size();
        if (ov > 0) {
            const tkz::TikTokenizer::Trimmed kept = tok.EncodeTrimPrefix(part, allowed, ov);
            next = p + part.size() - kept.second.size();
            if (kept.first.size() == n_ids) {                     // the whole chunk kept: its first item is dropped
                tkz::TikTokenizer::Trimmed first;
                for (int k = 1; first.first.empty(); ++k) first = tok.EncodeTrimSuffix(part, allowed, k);
                next = p + first.second.size();
            }
            if (next < p + part.size()) {                         // a chunk begun there that ends where this one does adds nothing
                const tkz::TikTokenizer::Trimmed trial = tok.EncodeTrimSuffix(text.substr(next), allowed, mx);
                if (next + trial.second.size() == p + part.size()) next = p + part.size();
            }
        }
        p = next;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string vocab = slurp(argv[1]);
    const std::string p1 = "'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+";
    const std::string EOT = "<|endoftext|>", IMS = "<|im_start|>", IME = "<|im_end|>";
    tkz::SpecialTokens specials = {{EOT, 50256}, {IMS, 50300}, {IME, 50301}};
    tkz::TikTokenizer tok(vocab, specials, p1);
    const std::vector<std::string> all = {EOT, IMS, IME}, only_end = {IME}, none;
    std::string longer;
    for (int k = 0; k < 600; ++k) longer += (k % 97 == 0) ? EOT : (k % 5 == 0 ? " it's" : (k % 7 == 0 ? " zqxjkv" : " token"));
    const std::string emoji = "\xF0\x9F\x98\x80";
    const std::vector<std::string> texts = {"", "Hello World", IMS + "Hello World" + IME, "Hello \xE2\xAD\x90 World" + IME, IME, " ", std::string(300, 'x'), IMS + IME, "a" + IMS,
                                            EOT + EOT + "x", emoji, "caf\xC3\xA9 " + emoji + emoji + " \xE6\xBC\xA2\xE5\xAD\x97", longer};
    const int budgets[][2] = {{1, 0}, {3, 1}, {3, 2}, {8, 3}, {64, 8}, {64, 63}};
    int loops = 0, spins = 0;
    for (const auto* allowed : {&all, &only_end, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatch(texts, *allowed);
        for (const auto& b : budgets) {
            const int mx = b[0], ov = b[1];
            const int64_t c0 = calls(tok);
            const std::vector<Chunks> batch = tok.EncodeChunksOverlapBatch(texts, *allowed, mx, ov);
            REQUIRE(calls(tok) == c0 + 1 && batch.size() == texts.size());
            for (size_t t = 0; t < texts.size(); ++t) {
                REQUIRE(well_formed(tok, texts[t], ids[t], batch[t], mx));
                REQUIRE(tok.EncodeChunksOverlap(texts[t], *allowed, mx, ov) == batch[t]);
                if (ov == 0) REQUIRE(batch[t] == tok.EncodeChunks(texts[t], *allowed, mx));
                Chunks loop;
                if (texts[t].size() > 200 && mx < 8) continue;     // (the loop is three calls a chunk: the long texts at the larger budgets only)
                if (trim_loop(tok, texts[t], *allowed, mx, ov, loop)) { REQUIRE(loop == batch[t]); ++loops; } else ++spins;
            }
        }
    }
    REQUIRE(loops > 100 && spins > 10);                       // (both kinds of text were met)
    REQUIRE(tok.EncodeChunksOverlap(longer, 64, 8).size() >= 3 && tok.EncodeChunksOverlap(longer, 64, 8) == tok.EncodeChunksOverlap(longer, all, 64, 8) &&
            tok.EncodeChunksOverlap(longer, 64, 8, false) == tok.EncodeChunksOverlap(longer, none, 64, 8));
    REQUIRE(tok.EncodeChunksOverlapBatch({}, none, 4, 1).empty() && tok.EncodeChunksOverlap("", 4, 1).empty());
    {   // consecutive chunks of plain words at (4, 2) share two tokens and their text
        const Chunks ch = tok.EncodeChunksOverlap(" token token token token token token token", none, 4, 2);
        REQUIRE(ch.size() == 3 && ch[0].second == " token token token token" && ch[1].second == ch[0].second && ch[2].second == " token token token");
    }
    const int bad[][2] = {{0, 0}, {-1, 0}, {3, -1}, {3, 3}, {3, 4}};
    for (const auto& b : bad) {                               // a budget below 1, an overlap outside [0, budget)
        bool refused = false;
        try { (void)tok.EncodeChunksOverlap("Hello World", none, b[0], b[1]); } catch (const tkz::Error&) { refused = true; }
        REQUIRE(refused);
        refused = false;
        try { (void)tok.EncodeChunksOverlapBatchUtf16({}, none, b[0], b[1]); } catch (const tkz::Error&) { refused = true; }
        REQUIRE(refused);
    }
    // std::u16string callers: texts sliced in code units -- a lone surrogate, a pair, a literal, an emoji the table splits
    std::vector<std::u16string> wide = {widen("Hello World"), widen(IMS + "Hello") + u" \xD83D\xDE00 " + widen(IME), std::u16string(u"lone \xD800 half"), u"", widen(longer),
                                        std::u16string(u"cut \xD83D"), std::u16string(u"\xDE00 here"), std::u16string(u"\xD83D\xDE00")};
    for (const auto* allowed : {&all, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatchUtf16(wide, *allowed);
        for (const auto& b : budgets) {
            const int mx = b[0], ov = b[1];
            const auto batch = tok.EncodeChunksOverlapBatchUtf16(wide, *allowed, mx, ov);
            for (size_t t = 0; t < wide.size(); ++t) {
                if (batch[t].empty()) { REQUIRE(ids[t].empty()); continue; }
                for (const auto& c : batch[t]) REQUIRE(!c.first.empty() && c.first.size() <= static_cast<size_t>(mx));
                // the first chunk starts the text and the last ends it; the ids start Encode's and end them
                const auto& f = batch[t].front();
                const auto& l = batch[t].back();
                REQUIRE(wide[t].compare(0, f.second.size(), f.second) == 0 && std::equal(f.first.begin(), f.first.end(), ids[t].begin()));
                REQUIRE(wide[t].size() >= l.second.size() && wide[t].compare(wide[t].size() - l.second.size(), l.second.size(), l.second) == 0);
                REQUIRE(ids[t].size() >= l.first.size() && std::equal(l.first.begin(), l.first.end(), ids[t].end() - static_cast<std::ptrdiff_t>(l.first.size())));
                REQUIRE(tok.EncodeChunksOverlapUtf16(wide[t], *allowed, mx, ov) == batch[t]);
                if (ov == 0) REQUIRE(batch[t] == tok.EncodeChunksUtf16(wide[t], *allowed, mx));
            }
        }
    }
    // a registered set the device path does not hold: no host path, the reference's NotImplementedException; nothing allowed is the plain call
    tkz::SpecialTokens many;
    for (int k = 0; k < 300; ++k) many.push_back({"<|s" + std::to_string(k) + "|>", 200000 + k});
    tkz::TikTokenizer tok2(vocab, many, p1);
    bool refused = false;
    try { (void)tok2.EncodeChunksOverlap("a<|s7|>b", {"<|s7|>"}, 2, 1); } catch (const tkz::NotImplementedError&) { refused = true; }
    REQUIRE(refused && well_formed(tok2, "a<|s7|>b", tok2.Encode("a<|s7|>b", false), tok2.EncodeChunksOverlap("a<|s7|>b", none, 2, 1), 2) && calls(tok2) == 1);
    std::printf("cpp chunks overlap ok\n");
    return 0;
}
