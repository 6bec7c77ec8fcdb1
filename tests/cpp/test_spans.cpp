// The span methods of the C++ host mirror (include/tkz_tokenizer.hpp) -- EncodeWithOffsets, EncodeWithOffsetsBatch and their Utf16 forms --, which call
// tkz_encode_batch_spans_utf8 / _utf16: the ids against Encode / EncodeBatch / EncodeUtf16 for the same arguments, the starts against the keys Decode returns for
// the ids (bytes) and against the units begun in front of every token (code units), with the calls read from tkz_encoder_spans_calls.  Built by
// tests/test_cpp_spans.py against the emulated library on CPU and against libtkz.so on the GPU.  argv: gpt2.tiktoken
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int64_t calls(const tkz::TikTokenizer& tok) { int64_t c = 0; tkz_encoder_spans_calls(tok.native(), &c); return c; }
static std::u16string widen(const std::string& ascii) { return std::u16string(ascii.begin(), ascii.end()); }
static int32_t units_begun(const std::string& s, size_t n) {
    int32_t u = 0;
    for (size_t i = 0; i < n; ++i) { const unsigned char c = static_cast<unsigned char>(s[i]); u += ((c & 0xC0) != 0x80) + (c >= 0xF0); }
    return u;
}
// the byte spans partition `text` into the keys of the ids
static bool partitions(const tkz::TikTokenizer& tok, const std::string& text, const tkz::TikTokenizer::TokenSpans& sp) {
    if (sp.ids.size() != sp.starts.size()) return false;
    size_t pos = 0;
    for (size_t t = 0; t < sp.ids.size(); ++t) {
        const std::string key = tok.Decode({sp.ids[t]});
        if (static_cast<size_t>(sp.starts[t]) != pos || text.compare(pos, key.size(), key) != 0) return false;
        pos += key.size();
    }
    return pos == text.size();
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
    for (const auto* allowed : {&all, &only_end, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatch(texts, *allowed);
        const int64_t c0 = calls(tok);
        const std::vector<tkz::TikTokenizer::TokenSpans> batch = tok.EncodeWithOffsetsBatch(texts, *allowed);
        REQUIRE(calls(tok) == c0 + 1 && batch.size() == texts.size());
        for (size_t t = 0; t < texts.size(); ++t) {
            REQUIRE(batch[t].ids == ids[t] && partitions(tok, texts[t], batch[t]));
            const tkz::TikTokenizer::TokenSpans one = tok.EncodeWithOffsets(texts[t], *allowed);
            REQUIRE(one.ids == batch[t].ids && one.starts == batch[t].starts);
        }
    }
    REQUIRE(tok.EncodeWithOffsetsBatch({}).empty() && tok.EncodeWithOffsets("").ids.empty());
    {   // an allowed literal is one token whose span is the literal
        const tkz::TikTokenizer::TokenSpans sp = tok.EncodeWithOffsets("ab" + EOT + "cd", all);
        size_t k = 0;
        while (k < sp.ids.size() && sp.ids[k] != 50256) ++k;
        REQUIRE(k + 1 < sp.ids.size() && sp.starts[k] == 2 && sp.starts[k + 1] == 2 + static_cast<int32_t>(EOT.size()));
    }
    // std::u16string callers: offsets in code units -- a lone surrogate, a pair, a literal, an emoji the table splits
    std::vector<std::u16string> wide = {widen("Hello World"), widen(IMS + "Hello") + u" \xD83D\xDE00 " + widen(IME), std::u16string(u"lone \xD800 half"), u"", widen(longer),
                                        std::u16string(u"cut \xD83D"), std::u16string(u"\xDE00 here"), std::u16string(u"\xD83D\xDE00")};
    for (const auto* allowed : {&all, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatchUtf16(wide, *allowed);
        const std::vector<tkz::TikTokenizer::TokenSpans> batch = tok.EncodeWithOffsetsBatchUtf16(wide, *allowed);
        for (size_t t = 0; t < wide.size(); ++t) {
            REQUIRE(batch[t].ids == ids[t] && batch[t].starts.size() == ids[t].size());
            // the units begun in front of every token, from the keys of the ids
            std::string bytes;
            for (size_t k = 0; k < ids[t].size(); ++k) {
                REQUIRE(batch[t].starts[k] == units_begun(bytes, bytes.size()));
                bytes += tok.Decode({ids[t][k]});
            }
            REQUIRE(units_begun(bytes, bytes.size()) == static_cast<int32_t>(wide[t].size()));
            const tkz::TikTokenizer::TokenSpans one = tok.EncodeWithOffsetsUtf16(wide[t], *allowed);
            REQUIRE(one.ids == batch[t].ids && one.starts == batch[t].starts);
        }
    }
    {   // the emoji: the first token carries both units, the others have empty unit spans
        const tkz::TikTokenizer::TokenSpans sp = tok.EncodeWithOffsetsUtf16(u"\xD83D\xDE00");
        REQUIRE(sp.ids.size() > 1 && sp.starts[0] == 0);
        for (size_t k = 1; k < sp.starts.size(); ++k) REQUIRE(sp.starts[k] == 2);
    }
    // a registered set the device path does not hold: no host path, the reference's NotImplementedException; nothing allowed is the plain call
    tkz::SpecialTokens many;
    for (int k = 0; k < 300; ++k) many.push_back({"<|s" + std::to_string(k) + "|>", 200000 + k});
    tkz::TikTokenizer tok2(vocab, many, p1);
    bool refused = false;
    try { (void)tok2.EncodeWithOffsets("a<|s7|>b", {"<|s7|>"}); } catch (const tkz::NotImplementedError&) { refused = true; }
    REQUIRE(refused && tok2.EncodeWithOffsets("a<|s7|>b").ids == tok2.Encode("a<|s7|>b", false) && calls(tok2) == 1);
    std::printf("cpp spans ok\n");
    return 0;
}
