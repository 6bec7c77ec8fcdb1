// The single-list Decode methods of the C++ host mirror (include/tkz_tokenizer.hpp) -- Decode(std::vector<int32_t>) and DecodeUtf16 --, which call
// tkz_decode_utf8 / tkz_decode_utf16: against the batch methods (DecodeBatch / DecodeBatchUtf16, the batch entries), with the route read from
// tkz_encoder_small_decode_calls.  Built by tests/test_cpp_small_decode.py against the emulated library on CPU and against libtkz.so on the GPU.
// argv: gpt2.tiktoken
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Route { int64_t calls, handed; };
static Route route(const tkz::TikTokenizer& tok) {
    Route r{0, 0};
    tkz_encoder_small_decode_calls(tok.native(), &r.calls, &r.handed);
    return r;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string vocab = slurp(argv[1]);
    const std::string p1 = "'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+";
    const std::string EOT = "<|endoftext|>", FAR = "<|\xF0\x9F\x98\x80 far|>";
    // (an id far above the vocabulary: the decode table's sparse form; its literal holds a 4-byte char)
    tkz::SpecialTokens specials = {{EOT, 50256}, {FAR, 5000000}};
    tkz::TikTokenizer tok(vocab, specials, p1);
    const std::vector<std::string> all = {EOT, FAR}, none;
    const std::vector<std::string> texts = {
        "Hello <|endoftext|> World and a tail", "na\xC3\xAFve \xE2\x86\x92 \xE4\xB8\xAD\xE6\x96\x87 \xF0\x9F\x98\x80 done", "x", FAR + " between " + FAR,
        std::string(3000, 'a') + " b"};
    std::vector<std::vector<int32_t>> lists;
    for (const auto& t : texts) lists.push_back(tok.Encode(t, all));
    lists.push_back({});                                                        // no ids: the empty string, nothing launched
    lists.push_back({-3, 2147483647, 60000, 5000001});                          // only unknown ids: the empty string, from the launch
    {   // a list that ends inside a char, as a trimmed list does, and one that starts inside it: ill-formed bytes, U+FFFD in the units
        std::vector<int32_t> ids = tok.Encode(texts[1], none);
        REQUIRE(ids.size() > 4);
        lists.push_back(std::vector<int32_t>(ids.begin(), ids.end() - 2));
        lists.push_back(std::vector<int32_t>(ids.begin() + 3, ids.end()));
    }
    {   // five id tiles (the 1024-thread workgroup), and a list beyond the block's 32,768 ids (the batch path: the counter does not move)
        std::vector<int32_t> five, beyond;
        for (int k = 0; k < 4100; ++k) five.push_back(lists[1][k % lists[1].size()]);
        for (int k = 0; k < 32769; ++k) beyond.push_back(lists[0][k % lists[0].size()]);
        lists.push_back(five);
        lists.push_back(beyond);
    }
    for (size_t k = 0; k < lists.size(); ++k) {
        const auto& ids = lists[k];
        const Route r0 = route(tok);
        const std::string s = tok.Decode(ids);
        const std::u16string w = tok.DecodeUtf16(ids);
        const Route r1 = route(tok);
        const bool launch = !ids.empty() && ids.size() <= 32768;
        REQUIRE(r1.calls - r0.calls == (launch ? 2 : 0) && r1.handed == r0.handed);
        REQUIRE(s == tok.DecodeBatch({ids})[0]);
        REQUIRE(w == tok.DecodeBatchUtf16({ids})[0]);
        const Route r2 = route(tok);
        REQUIRE(r2.calls == r1.calls);                                          // (the batch methods are the batch entries still)
        if (k < texts.size()) REQUIRE(s == texts[k]);
        if (ids.empty() || k == 6) REQUIRE(s.empty() && w.empty());
    }
    REQUIRE(tok.DecodeUtf16(lists[3]).find(u"\xD83D\xDE00") != std::u16string::npos);      // the literal's 4-byte char is a pair
    {   // 1,100 ids of the longest key (128 bytes): more than the block's 131,072 bytes -- the launch hands the list back, the batch path answers; the
        // first capacity of the mirror (8 items an id) is short: each method calls twice
        int32_t longest = -1; size_t len = 0;
        std::vector<std::vector<int32_t>> every;
        for (int32_t id = 0; id < 50256; ++id) every.push_back({id});
        const std::vector<std::string> keys = tok.DecodeBatch(every);
        for (int32_t id = 0; id < 50256; ++id) if (keys[id].size() > len) { len = keys[id].size(); longest = id; }
        REQUIRE(len == 128);
        const std::vector<int32_t> ids(1100, longest);
        const Route r0 = route(tok);
        const std::string s = tok.Decode(ids);
        const std::u16string w = tok.DecodeUtf16(ids);
        const Route r1 = route(tok);
        REQUIRE(s.size() == 1100 * 128 && s == tok.DecodeBatch({ids})[0] && w == tok.DecodeBatchUtf16({ids})[0]);
        REQUIRE(r1.calls - r0.calls == 4 && r1.handed - r0.handed == 4);
    }
    std::printf("cpp small decode ok\n");
    return 0;
}
