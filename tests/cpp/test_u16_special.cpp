// The std::u16string methods of the C++ host mirror (include/tkz_tokenizer.hpp) -- EncodeBatchFlatUtf16 / EncodeBatchUtf16 / EncodeUtf16 with allowedSpecial,
// EncodeTrimSuffixBatchUtf16 / EncodeTrimPrefixBatchUtf16 -- against the header's own host walk over the code units, text by text: well-formed text, a real
// U+FFFD under a literal that holds one, and lone surrogates under it (the device may not take the literal there: .NET searches the string).  Built by
// tests/test_emu_u16_special.py against the emulated library on CPU and by tests/test_gpu_u16_special.py against libtkz.so.  argv: gpt2.tiktoken
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string vocab = slurp(argv[1]);
    const std::string p1 = "'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+";
    const std::string A = "x\xEF\xBF\xBD", B = "x", C = "<\xEF\xBF\xBD>", EOT = "<|endoftext|>";
    tkz::SpecialTokens specials = {{A, 60001}, {B, 60002}, {C, 60003}, {EOT, 50256}};
    tkz::TikTokenizer tok(vocab, specials, p1);
    const char16_t HI = 0xD83D, LO = 0xDE00;
    std::vector<std::u16string> texts = {
        u"a x", u"a x� b", u"a <", u"", u"Hello <|endoftext|> World \U0001F600 漢字<|endoftext|>", u"a <�> b", u"plain text only",
        u"tail x", std::u16string(1500, u'a') + u" end<|endoftext|>"};
    texts[0] += HI; texts[0] += u" b";                       // `x` + a lone high half: A on bytes, B (or plain text) on the string
    texts[2] += LO; texts[2] += u"> b";                      // `<` + a lone low half + `>`: plain text
    texts[7] += HI;                                          // a high half that ends its text (the next one does not start with a low half: still alone)
    const std::vector<std::string> all = {A, B, C, EOT}, onlyA = {A}, ac = {A, C, EOT}, none;
    for (const auto* allowed : {&all, &onlyA, &ac, &none}) {
        tkz::FlatBatch fb;
        tok.EncodeBatchFlatUtf16(texts, *allowed, fb, 2);
        const auto batch = tok.EncodeBatchUtf16(texts, *allowed);
        REQUIRE(fb.n_texts() == static_cast<int64_t>(texts.size()) && batch.size() == texts.size());
        for (size_t t = 0; t < texts.size(); ++t) {
            const std::vector<int32_t> want = tok.encode_host16(texts[t], *allowed);
            REQUIRE(fb.text(static_cast<int64_t>(t)) == want);
            REQUIRE(batch[t] == want);
        }
        REQUIRE(tok.EncodeUtf16(texts[0], *allowed) == tok.encode_host16(texts[0], *allowed));
        for (int mx = -1; mx <= 12; ++mx) {
            const auto s = tok.EncodeTrimSuffixBatchUtf16(texts, *allowed, mx), p = tok.EncodeTrimPrefixBatchUtf16(texts, *allowed, mx);
            REQUIRE(s.size() == texts.size() && p.size() == texts.size());
            for (size_t t = 0; t < texts.size(); ++t) {
                REQUIRE(s[t] == tok.trim_suffix_host16(texts[t], *allowed, mx));
                REQUIRE(p[t] == tok.trim_prefix_host16(texts[t], *allowed, mx));
                REQUIRE(mx < 0 || static_cast<int>(s[t].first.size()) <= mx);
            }
        }
    }
    // the lone surrogate, spelled out: with only A allowed no special id appears; with everything allowed it is B; the real U+FFFD gives A
    auto has = [](const std::vector<int32_t>& v, int32_t id) { for (int32_t x : v) if (x == id) return true; return false; };
    REQUIRE(!has(tok.EncodeUtf16(texts[0], onlyA), 60001));
    REQUIRE(has(tok.EncodeUtf16(texts[0], all), 60002) && !has(tok.EncodeUtf16(texts[0], all), 60001));
    REQUIRE(has(tok.EncodeUtf16(texts[1], onlyA), 60001));
    REQUIRE(!has(tok.EncodeUtf16(texts[2], all), 60003) && has(tok.EncodeUtf16(texts[5], all), 60003));
    // the bool form, the plain form, an empty batch
    tkz::FlatBatch f1, f2;
    tok.EncodeBatchFlatUtf16(texts, true, f1);
    tok.EncodeBatchFlatUtf16(texts, all, f2);
    REQUIRE(f1.n_ids() == f2.n_ids() && std::equal(f1.ids(), f1.ids() + f1.n_ids(), f2.ids()));
    tok.EncodeBatchFlatUtf16(texts, false, f1);
    tok.EncodeBatchFlatUtf16(texts, f2);
    REQUIRE(f1.n_ids() == f2.n_ids() && std::equal(f1.ids(), f1.ids() + f1.n_ids(), f2.ids()));
    REQUIRE(tok.EncodeTrimSuffixBatchUtf16({}, all, 3).empty());
    // a registered set beyond the device path (257 literals): the host walk answers, and agrees with itself through every method
    tkz::SpecialTokens many;
    for (int i = 0; i < 257; ++i) many.push_back({"<|s" + std::to_string(i) + "|>", 70000 + i});
    tkz::TikTokenizer tok2(vocab, many, p1);
    const std::vector<std::u16string> t2 = {u"a<|s7|>b <|s256|><|s30|", u"x"};
    const std::vector<std::string> a2 = {"<|s7|>", "<|s256|>"};
    const auto r2 = tok2.EncodeBatchUtf16(t2, a2);
    REQUIRE(r2[0] == tok2.encode_host16(t2[0], a2) && has(r2[0], 70007) && has(r2[0], 70256));
    REQUIRE(tok2.EncodeTrimSuffixBatchUtf16(t2, a2, 3)[0] == tok2.trim_suffix_host16(t2[0], a2, 3));
    REQUIRE(tok2.EncodeTrimPrefixBatchUtf16(t2, a2, 2)[0] == tok2.trim_prefix_host16(t2[0], a2, 2));
    std::printf("cpp u16 special ok\n");
    return 0;
}
