// The chunk methods of the C++ host mirror (include/tkz_tokenizer.hpp) -- EncodeChunks, EncodeChunksBatch and their Utf16 forms --, which call
// tkz_encode_batch_chunks_utf8 / _utf16: the ids against Encode / EncodeUtf16 for the same arguments, the chunks against the caller's own loop over
// EncodeTrimSuffix (while no piece exceeds the budget the two are the same, ids and texts), the byte texts against the keys Decode returns for the ids, the
// code-unit texts against the units begun in front of every chunk, with the calls read from tkz_encoder_chunks_calls.  Built by tests/test_cpp_chunks.py against
// the emulated library on CPU and against libtkz.so on the GPU.  argv: gpt2.tiktoken
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using Chunks = std::vector<tkz::TikTokenizer::Trimmed>;
static int64_t calls(const tkz::TikTokenizer& tok) { int64_t c = 0; tkz_encoder_chunks_calls(tok.native(), &c); return c; }
static std::u16string widen(const std::string& ascii) { return std::u16string(ascii.begin(), ascii.end()); }
static size_t units_begun(const std::string& s) {
    size_t u = 0;
    for (unsigned char c : s) u += ((c & 0xC0) != 0x80) + (c >= 0xF0);
    return u;
}
// the chunks partition the ids of Encode and the bytes of `text`, every chunk's text is the keys of its ids, and no chunk is empty or over the budget
static bool partitions(const tkz::TikTokenizer& tok, const std::string& text, const std::vector<int32_t>& ids, const Chunks& ch, int mx) {
    std::vector<int32_t> all;
    std::string joined;
    for (const auto& c : ch) {
        if (c.first.empty() || c.first.size() > static_cast<size_t>(mx) || tok.Decode(c.first) != c.second) return false;
        all.insert(all.end(), c.first.begin(), c.first.end());
        joined += c.second;
    }
    return all == ids && joined == text;
}
// the caller's loop; false when it would spin (the next piece alone exceeds the budget)
static bool trim_loop(const tkz::TikTokenizer& tok, std::string rest, const std::vector<std::string>& allowed, int mx, Chunks& out) {
    while (!rest.empty()) {
        tkz::TikTokenizer::Trimmed t = tok.EncodeTrimSuffix(rest, allowed, mx);
        if (t.first.empty()) return false;
        rest = rest.substr(t.second.size());
        out.push_back(std::move(t));
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
    for (int k = 0; k < 3000; ++k) longer += (k % 97 == 0) ? EOT : (k % 5 == 0 ? " it's" : (k % 7 == 0 ? " zqxjkv" : " token"));
    const std::string emoji = "\xF0\x9F\x98\x80";
    const std::vector<std::string> texts = {"", "Hello World", IMS + "Hello World" + IME, "Hello \xE2\xAD\x90 World" + IME, IME, " ", std::string(300, 'x'), IMS + IME, "a" + IMS,
                                            "<|im_start", EOT + EOT + "x", emoji, "caf\xC3\xA9 " + emoji + emoji + " \xE6\xBC\xA2\xE5\xAD\x97", longer};
    int loops = 0, spins = 0;
    for (const auto* allowed : {&all, &only_end, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatch(texts, *allowed);
        for (int mx : {1, 3, 8, 64}) {
            const int64_t c0 = calls(tok);
            const std::vector<Chunks> batch = tok.EncodeChunksBatch(texts, *allowed, mx);
            REQUIRE(calls(tok) == c0 + 1 && batch.size() == texts.size());
            for (size_t t = 0; t < texts.size(); ++t) {
                REQUIRE(partitions(tok, texts[t], ids[t], batch[t], mx));
                REQUIRE(tok.EncodeChunks(texts[t], *allowed, mx) == batch[t]);
                Chunks loop;
                if (trim_loop(tok, texts[t], *allowed, mx, loop)) { REQUIRE(loop == batch[t]); ++loops; } else ++spins;
            }
        }
    }
    REQUIRE(loops > 100 && spins > 10);                       // (both kinds of text were met)
    REQUIRE(tok.EncodeChunks(longer, 64).size() >= 3 && tok.EncodeChunks(longer, 64) == tok.EncodeChunks(longer, all, 64) && tok.EncodeChunks(longer, 64, false) == tok.EncodeChunks(longer, none, 64));
    REQUIRE(tok.EncodeChunksBatch({}, none, 4).empty() && tok.EncodeChunks("", 4).empty());
    {   // an allowed literal is one item of one token: at max 1 it is a chunk of its own whose text is the literal
        const Chunks ch = tok.EncodeChunks("ab" + EOT + "cd", all, 1);
        size_t k = 0;
        while (k < ch.size() && ch[k].first[0] != 50256) ++k;
        REQUIRE(k + 1 < ch.size() && ch[k].second == EOT);
    }
    for (int bad : {0, -1}) {                                 // a budget below 1
        bool refused = false;
        try { (void)tok.EncodeChunks("Hello World", none, bad); } catch (const tkz::Error&) { refused = true; }
        REQUIRE(refused);
    }
    // std::u16string callers: texts sliced in code units -- a lone surrogate, a pair, a literal, an emoji the table splits
    std::vector<std::u16string> wide = {widen("Hello World"), widen(IMS + "Hello") + u" \xD83D\xDE00 " + widen(IME), std::u16string(u"lone \xD800 half"), u"", widen(longer),
                                        std::u16string(u"cut \xD83D"), std::u16string(u"\xDE00 here"), std::u16string(u"\xD83D\xDE00")};
    for (const auto* allowed : {&all, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatchUtf16(wide, *allowed);
        for (int mx : {1, 5}) {
            const auto batch = tok.EncodeChunksBatchUtf16(wide, *allowed, mx);
            for (size_t t = 0; t < wide.size(); ++t) {
                std::vector<int32_t> joined_ids;
                std::u16string joined;
                std::string bytes;
                for (const auto& c : batch[t]) {
                    REQUIRE(!c.first.empty() && c.first.size() <= static_cast<size_t>(mx));
                    REQUIRE(joined.size() == units_begun(bytes));      // the chunk starts at the units begun in front of it
                    joined_ids.insert(joined_ids.end(), c.first.begin(), c.first.end());
                    joined += c.second;
                    bytes += tok.Decode(c.first);
                }
                REQUIRE(joined_ids == ids[t] && joined == wide[t]);
                REQUIRE(tok.EncodeChunksUtf16(wide[t], *allowed, mx) == batch[t]);
            }
        }
    }
    {   // the emoji at max 1: the first chunk carries both units, the others are empty strings
        const auto ch = tok.EncodeChunksUtf16(u"\xD83D\xDE00", none, 1);
        REQUIRE(ch.size() > 1 && ch[0].second.size() == 2);
        for (size_t k = 1; k < ch.size(); ++k) REQUIRE(ch[k].second.empty() && ch[k].first.size() == 1);
    }
    // a registered set the device path does not hold: no host path, the reference's NotImplementedException; nothing allowed is the plain call
    tkz::SpecialTokens many;
    for (int k = 0; k < 300; ++k) many.push_back({"<|s" + std::to_string(k) + "|>", 200000 + k});
    tkz::TikTokenizer tok2(vocab, many, p1);
    bool refused = false;
    try { (void)tok2.EncodeChunks("a<|s7|>b", {"<|s7|>"}, 2); } catch (const tkz::NotImplementedError&) { refused = true; }
    REQUIRE(refused && partitions(tok2, "a<|s7|>b", tok2.Encode("a<|s7|>b", false), tok2.EncodeChunks("a<|s7|>b", none, 2), 2) && calls(tok2) == 1);
    std::printf("cpp chunks ok\n");
    return 0;
}
