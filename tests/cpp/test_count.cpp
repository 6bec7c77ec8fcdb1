// The count methods of the C++ host mirror (include/tkz_tokenizer.hpp) -- CountTokens, CountTokensBatch and their Utf16 forms --, which call tkz_count_utf8 /
// _utf16 and tkz_count_batch_utf8 / _utf16: against the sizes of what Encode / EncodeBatch / EncodeUtf16 / EncodeBatchUtf16 return for the same arguments, with
// the route read from tkz_encoder_count_calls.  Built by tests/test_cpp_count.py against the emulated library on CPU and against libtkz.so on the GPU.
// argv: gpt2.tiktoken
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Calls { int64_t calls, single; };
static Calls calls(const tkz::TikTokenizer& tok) {
    Calls c{0, 0};
    tkz_encoder_count_calls(tok.native(), &c.calls, &c.single);
    return c;
}
// calls the single-launch kernel answered (those it handed back to the batch path not counted)
static int64_t launches(const tkz::TikTokenizer& tok) {
    int64_t c = 0, h = 0;
    tkz_encoder_small_path_calls(tok.native(), &c, &h);
    return c - h;
}
static std::u16string widen(const std::string& ascii) { return std::u16string(ascii.begin(), ascii.end()); }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string vocab = slurp(argv[1]);
    const std::string p1 = "'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+";
    const std::string EOT = "<|endoftext|>", IMS = "<|im_start|>", IME = "<|im_end|>";
    tkz::SpecialTokens specials = {{EOT, 50256}, {IMS, 50300}, {IME, 50301}};
    tkz::TikTokenizer tok(vocab, specials, p1);
    const std::vector<std::string> all = {EOT, IMS, IME}, only_end = {IME}, none;
    std::string longer;
    for (int k = 0; k < 9000; ++k) longer += (k % 97 == 0) ? EOT : (k % 5 == 0 ? " it's" : " token");           // beyond a sub-tile, literals inside: the batch path beside the launch
    std::string beyond(140000, 'a');                                                                            // beyond the single launch: the batch path
    for (size_t k = 7; k < beyond.size(); k += 8) beyond[k] = ' ';
    const std::vector<std::string> texts = {"", "Hello World", IMS + "Hello World" + IME, "Hello \xE2\xAD\x90 World" + IME, IME, " ", std::string(300, 'x'),
                                            IMS + IME, "a" + IMS, "<|im_start", EOT + EOT + "x", longer};
    for (const auto* allowed : {&all, &only_end, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatch(texts, *allowed);
        std::vector<int64_t> sizes;
        const int64_t e0 = launches(tok);
        for (const auto& t : texts) sizes.push_back(static_cast<int64_t>(tok.Encode(t, *allowed).size()));
        const int64_t e1 = launches(tok);
        const Calls c0 = calls(tok);
        const std::vector<int64_t> counts = tok.CountTokensBatch(texts, *allowed);
        const Calls cb = calls(tok);
        const int64_t eb = launches(tok);
        REQUIRE(counts.size() == texts.size());
        for (size_t t = 0; t < texts.size(); ++t) {
            REQUIRE(counts[t] == static_cast<int64_t>(ids[t].size()));
            REQUIRE(tok.CountTokens(texts[t], *allowed) == sizes[t]);
        }
        const Calls c1 = calls(tok);
        REQUIRE(c1.calls - c0.calls == 1 + static_cast<int64_t>(texts.size()));
        // the single texts take the launch exactly where the Encode calls did (most of them), and the second counter says so; a batch with literals never takes it
        REQUIRE(c1.single - cb.single == e1 - e0 && e1 - e0 >= 9 && launches(tok) - eb == c1.single - cb.single);
        REQUIRE(cb.single - c0.single == eb - e1 && (allowed == &none || eb == e1));
    }
    REQUIRE(tok.CountTokens(texts[2]) == static_cast<int64_t>(tok.Encode("Hello World", false).size()) + 2);       // (applySpecialTokens = true)
    REQUIRE(tok.CountTokens(texts[2], false) == static_cast<int64_t>(tok.Encode(texts[2], false).size()) && tok.CountTokens(texts[2], false) > tok.CountTokens(texts[2]));
    REQUIRE(tok.CountTokensBatch(texts) == tok.CountTokensBatch(texts, all) && tok.CountTokensBatch(texts, false) == tok.CountTokensBatch(texts, none));
    REQUIRE(tok.CountTokensBatch({}).empty() && tok.CountTokens("") == 0);
    REQUIRE(tok.CountTokens(beyond, false) == static_cast<int64_t>(tok.Encode(beyond, false).size()));
    // std::u16string callers: a lone surrogate, a pair, a literal
    std::vector<std::u16string> wide = {widen("Hello World"), widen(IMS + "Hello") + u" \xD83D\xDE00 " + widen(IME), std::u16string(u"lone \xD800 half"), u"", widen(longer)};
    wide.push_back(std::u16string(u"cut \xD83D"));
    wide.push_back(std::u16string(u"\xDE00 here"));
    for (const auto* allowed : {&all, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatchUtf16(wide, *allowed);
        const std::vector<int64_t> counts = tok.CountTokensBatchUtf16(wide, *allowed);
        for (size_t t = 0; t < wide.size(); ++t) {
            REQUIRE(counts[t] == static_cast<int64_t>(ids[t].size()));
            REQUIRE(tok.CountTokensUtf16(wide[t], *allowed) == static_cast<int64_t>(tok.EncodeUtf16(wide[t], *allowed).size()));
        }
    }
    REQUIRE(tok.CountTokensBatchUtf16({}).empty() && tok.CountTokensUtf16(u"") == 0);
    // a registered set the device path does not hold: the counts are the host segmentation's
    tkz::SpecialTokens many;
    for (int k = 0; k < 300; ++k) many.push_back({"<|s" + std::to_string(k) + "|>", 200000 + k});
    tkz::TikTokenizer tok2(vocab, many, p1);
    const std::string t = "a<|s7|>b <|s299|><|s30|";
    REQUIRE(tok2.CountTokens(t) == static_cast<int64_t>(tok2.Encode(t).size()) && tok2.CountTokens(t, false) == static_cast<int64_t>(tok2.Encode(t, false).size()));
    REQUIRE(tok2.CountTokensBatch({t, "", t})[2] == static_cast<int64_t>(tok2.Encode(t).size()));
    REQUIRE(calls(tok2).calls == 1);                                                   // (the plain call: the refused ones are not counted)
    std::printf("cpp count ok\n");
    return 0;
}
