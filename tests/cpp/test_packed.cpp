// The packed-rows method of the C++ host mirror (include/tkz_tokenizer.hpp) -- EncodeBatchPacked for std::string and std::u16string --, which calls
// tkz_encode_batch_packed_utf8 / _utf16: held against the rule of tkz.h applied here to the ids EncodeBatch / EncodeBatchUtf16 return for the same arguments
// (those methods are held against the oracle by their own tests), with the calls read from tkz_encoder_packed_calls.  Built by tests/test_cpp_packed.py against
// the emulated library on CPU and against libtkz.so on the GPU.  argv: gpt2.tiktoken
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using Rows = tkz::TikTokenizer::PackedRows;
static int64_t calls(const tkz::TikTokenizer& tok) { int64_t c = 0; tkz_encoder_packed_calls(tok.native(), &c); return c; }
static std::u16string widen(const std::string& ascii) { return std::u16string(ascii.begin(), ascii.end()); }

// the rule of tkz.h over the ids of every document
static Rows rule(const std::vector<std::vector<int32_t>>& docs, int64_t L, int32_t bos, int32_t eos, int32_t pad) {
    Rows r;
    r.row_len = L;
    std::vector<int32_t> stream;
    r.doc_offsets.push_back(0);
    for (const auto& d : docs) {
        if (bos >= 0) stream.push_back(bos);
        stream.insert(stream.end(), d.begin(), d.end());
        if (eos >= 0) stream.push_back(eos);
        r.doc_offsets.push_back(static_cast<int64_t>(stream.size()));
    }
    const int64_t T = static_cast<int64_t>(stream.size());
    r.total_tokens = T;
    r.n_rows = (T + L - 1) / L;
    r.ids.assign(static_cast<size_t>(r.n_rows * L), pad);
    std::copy(stream.begin(), stream.end(), r.ids.begin());
    r.pos.assign(r.ids.size(), 0);
    size_t d = 0;
    int64_t last = 0;
    for (int64_t t = 0; t < T; ++t) {
        bool start = t % L == 0;
        while (d + 1 < r.doc_offsets.size() && r.doc_offsets[d] < t) ++d;
        for (size_t k = d; k + 1 < r.doc_offsets.size() && r.doc_offsets[k] == t; ++k) if (r.doc_offsets[k + 1] > t) start = true;
        if (start) { r.seg_starts.push_back(t); last = t; }
        r.pos[static_cast<size_t>(t)] = static_cast<int32_t>(t - last);
    }
    r.seg_starts.push_back(T);
    return r;
}
static bool same(const Rows& a, const Rows& b) {
    return a.row_len == b.row_len && a.n_rows == b.n_rows && a.total_tokens == b.total_tokens && a.ids == b.ids && a.pos == b.pos && a.seg_starts == b.seg_starts &&
           a.doc_offsets == b.doc_offsets;
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
    const std::vector<std::string> texts = {"", "Hello World", IMS + "Hello World" + IME, "", "", IME, " ", std::string(300, 'x'), "a" + IMS, EOT + EOT + "x", emoji,
                                            "caf\xC3\xA9 " + emoji + emoji + " \xE6\xBC\xA2\xE5\xAD\x97", longer, ""};
    REQUIRE(tok.SpecialTokenId(EOT) == 50256);
    for (const auto* allowed : {&all, &only_end, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatch(texts, *allowed);
        for (int64_t L : {1, 7, 512, 100000}) {
            const int32_t frames[4][2] = {{-1, -1}, {11, -1}, {-1, tok.SpecialTokenId(EOT)}, {11, 50256}};
            for (const auto& fr : frames) {
                const int64_t c0 = calls(tok);
                const Rows got = tok.EncodeBatchPacked(texts, L, *allowed, fr[0], fr[1], -1);
                REQUIRE(calls(tok) == c0 + 1);
                REQUIRE(same(got, rule(ids, L, fr[0], fr[1], -1)));
            }
        }
    }
    {   // the worked example of tkz.h: documents of 3, 0 and 2 tokens, eos only
        const std::vector<std::string> ex = {" the of and", "", " to in"};
        const Rows a = tok.EncodeBatchPacked(ex, 4, none, -1, 9), b = tok.EncodeBatchPacked(ex, 3, none, -1, 9, 77);
        REQUIRE(a.total_tokens == 8 && a.n_rows == 2 && (a.seg_starts == std::vector<int64_t>{0, 4, 5, 8}) && (a.pos == std::vector<int32_t>{0, 1, 2, 3, 0, 0, 1, 2}));
        REQUIRE(b.n_rows == 3 && (b.seg_starts == std::vector<int64_t>{0, 3, 4, 5, 6, 8}) && (b.pos == std::vector<int32_t>{0, 1, 2, 0, 0, 0, 0, 1, 0}) && b.ids[8] == 77);
        REQUIRE((a.doc_offsets == std::vector<int64_t>{0, 4, 5, 8}) && a.ids[3] == 9 && a.ids[4] == 9 && a.ids[7] == 9);
    }
    {   // no texts; texts that are all empty
        const Rows e0 = tok.EncodeBatchPacked(std::vector<std::string>{}, 4, none, 1, 2);
        REQUIRE(e0.n_rows == 0 && e0.ids.empty() && e0.seg_starts == std::vector<int64_t>{0} && e0.doc_offsets == std::vector<int64_t>{0});
        const Rows e3 = tok.EncodeBatchPacked(std::vector<std::string>{"", "", ""}, 4, none, 1, 2, 5);
        REQUIRE(same(e3, rule({{}, {}, {}}, 4, 1, 2, 5)) && e3.total_tokens == 6 && e3.ids[7] == 5);
        const Rows z3 = tok.EncodeBatchPacked(std::vector<std::string>{"", "", ""}, 4);
        REQUIRE(z3.n_rows == 0 && z3.total_tokens == 0 && z3.seg_starts == std::vector<int64_t>{0});
    }
    for (int64_t bad : {int64_t(0), int64_t(-1), int64_t(1) << 31}) {            // a row length out of range; a framing id below -1
        bool refused = false;
        try { (void)tok.EncodeBatchPacked(texts, bad); } catch (const tkz::Error&) { refused = true; }
        REQUIRE(refused);
    }
    {
        bool refused = false;
        try { (void)tok.EncodeBatchPacked(texts, 8, none, -2); } catch (const tkz::Error&) { refused = true; }
        REQUIRE(refused);
        refused = false;
        try { (void)tok.SpecialTokenId("<|nope|>"); } catch (const tkz::Error&) { refused = true; }
        REQUIRE(refused);
    }
    // std::u16string callers: a lone surrogate, a pair, a pair cut by a document boundary, a literal
    std::vector<std::u16string> wide = {widen("Hello World"), widen(IMS + "Hello") + u" \xD83D\xDE00 " + widen(IME), std::u16string(u"lone \xD800 half"), u"", widen(longer),
                                        std::u16string(u"cut \xD83D"), std::u16string(u"\xDE00 here"), std::u16string(u"\xD83D\xDE00")};
    for (const auto* allowed : {&all, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatchUtf16(wide, *allowed);
        for (int64_t L : {5, 2048}) REQUIRE(same(tok.EncodeBatchPacked(wide, L, *allowed, 11, 50256, 3), rule(ids, L, 11, 50256, 3)));
        REQUIRE(same(tok.EncodeBatchPacked(wide, 64, *allowed), rule(ids, 64, -1, -1, 0)));
    }
    // a registered set the device path does not hold: no host path, the reference's NotImplementedException; nothing allowed is the plain call
    tkz::SpecialTokens many;
    for (int k = 0; k < 300; ++k) many.push_back({"<|s" + std::to_string(k) + "|>", 200000 + k});
    tkz::TikTokenizer tok2(vocab, many, p1);
    bool refused = false;
    try { (void)tok2.EncodeBatchPacked(std::vector<std::string>{"a<|s7|>b"}, 4, {"<|s7|>"}); } catch (const tkz::NotImplementedError&) { refused = true; }
    REQUIRE(refused && tok2.EncodeBatchPacked(std::vector<std::string>{"a<|s7|>b"}, 4).total_tokens == static_cast<int64_t>(tok2.Encode("a<|s7|>b", false).size()) && calls(tok2) == 1);
    std::printf("cpp packed ok\n");
    return 0;
}
