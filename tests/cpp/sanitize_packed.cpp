// A stand-alone driver for a sanitizer build of the host code behind the packed entries (tkz_encode_batch_packed_device / _utf8 / _utf16) and of k_pack_count /
// k_pack_write: tests/test_cpp_packed.py compiles it with the product sources and the CPU SIMT emulator (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under
// -fsanitize=address,undefined and runs it; nothing is loaded into an interpreter.  It walks the shapes of tests/packed_cases.py -- the four framing forms over
// runs of empty documents, row lengths from 1 to ten times the stream, streams at the tile edges, a document over three tiles, 300 documents in one tile, a
// literal allowed and not, the UTF-16 entry with lone surrogates, the argument rows and the empty batches -- twice over one encoder, with buffers of EXACTLY the
// capacities the rule gives (a store one past the end is the sanitizer's to find), one short of them, and without pos and seg_starts.  Every result is held
// against the rule of tkz.h applied to the ids and offsets of the matching encode entry.  argv: gpt2.tiktoken
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tkz.h"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, tkz_last_error()); return 1; } } while (0)

static const int64_t K = 2048;                               // kPackTile
static uint32_t g_rng = 2463534242u;
static uint32_t rnd(uint32_t n) { g_rng = g_rng * 1664525u + 1013904223u; return (g_rng >> 8) % n; }
static const char* kWords[] = {"the", "of", "and", "to", "in", "is", "that", "for", "it", "with", "as", "was", "on", "be", "at", "by", "this", "had", "not", "are"};
static std::string words(int64_t n) { std::string s; for (int64_t k = 0; k < n; ++k) { s += ' '; s += kWords[rnd(20)]; } return s; }      // n tokens

struct Batch { std::vector<uint8_t> bytes; std::vector<int64_t> offs{0}; void add(const std::string& d) { bytes.insert(bytes.end(), d.begin(), d.end()); offs.push_back((int64_t)bytes.size()); } };
struct Rows { int64_t T = 0, n_rows = 0; std::vector<int32_t> ids, pos; std::vector<int64_t> seg, offs; };

// the rule of tkz.h over the unframed ids and offsets
static Rows rule(const std::vector<int32_t>& ids, const std::vector<int64_t>& O, int64_t L, int32_t bos, int32_t eos, int32_t pad) {
    Rows r;
    const int64_t n = (int64_t)O.size() - 1, f = (bos >= 0) + (eos >= 0);
    r.T = O[(size_t)n] + f * n; r.n_rows = (r.T + L - 1) / L;
    r.ids.assign((size_t)(r.n_rows * L), pad); r.pos.assign((size_t)(r.n_rows * L), 0);
    std::vector<char> start((size_t)r.T + 1, 0);
    for (int64_t t = 0; t < r.T; t += L) start[(size_t)t] = 1;
    for (int64_t d = 0; d <= n; ++d) r.offs.push_back(O[(size_t)d] + f * d);
    for (int64_t d = 0; d < n; ++d) {
        int64_t t = r.offs[(size_t)d];
        if (r.offs[(size_t)d + 1] > t) start[(size_t)t] = 1;
        if (bos >= 0) r.ids[(size_t)t++] = bos;
        for (int64_t k = O[(size_t)d]; k < O[(size_t)d + 1]; ++k) r.ids[(size_t)t++] = ids[(size_t)k];
        if (eos >= 0) r.ids[(size_t)t++] = eos;
    }
    int64_t last = 0;
    for (int64_t t = 0; t < r.T; ++t) { if (start[(size_t)t]) { r.seg.push_back(t); last = t; } r.pos[(size_t)t] = (int32_t)(t - last); }
    r.seg.push_back(r.T);
    return r;
}

// the device entry (the emulated build's device memory is host memory) with buffers of exactly n_rows * L, n_segs + 1 and n_docs + 1 entries; without either
// array; one entry short; the host entry
static bool check_batch(tkz_encoder* e, const Batch& b, int64_t L, int32_t bos, int32_t eos) {
    const int64_t n = (int64_t)b.offs.size() - 1, total = b.offs.back();
    void* aligned = nullptr;                                                     // (d_bytes: 16-byte aligned)
    if (tkz_host_alloc((size_t)total + 64, &aligned) != TKZ_OK) return false;
    std::memset(aligned, 0, (size_t)total + 64);
    if (total) std::memcpy(aligned, b.bytes.data(), (size_t)total);
    const uint8_t* d = static_cast<const uint8_t*>(aligned);
    std::vector<int32_t> want_ids((size_t)total + 1);
    std::vector<int64_t> want((size_t)n + 1, 0);
    int64_t tw = 0;
    bool ok = n == 0 || tkz_encode_batch_device(e, d, b.offs.data(), n, total, want_ids.data(), total, want.data(), nullptr, &tw) == TKZ_OK;
    if (!ok) { tkz_host_free(aligned); return false; }
    const Rows R = rule(want_ids, want, L, bos, eos, -3);
    const int64_t cap = R.n_rows * L, nseg = (int64_t)R.seg.size() - 1;
    std::vector<int32_t> ids((size_t)cap, -9), pos((size_t)cap, -9);
    std::vector<int64_t> seg((size_t)nseg + 1, -9), offs((size_t)n + 1, -9);
    int64_t T = -1, rows = -1, segs = -1;
    ok = tkz_encode_batch_packed_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, -3, ids.data(), cap, offs.data(), pos.data(), seg.data(), nseg, nullptr, &T, &rows, &segs) == TKZ_OK;
    ok = ok && T == R.T && rows == R.n_rows && segs == nseg && ids == R.ids && pos == R.pos && seg == R.seg && offs == R.offs;
    std::fill(ids.begin(), ids.end(), -9);
    ok = ok && tkz_encode_batch_packed_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, -3, ids.data(), cap, offs.data(), nullptr, nullptr, 0, nullptr, &T, &rows, &segs) == TKZ_OK;
    ok = ok && ids == R.ids && segs == nseg;
    std::fill(pos.begin(), pos.end(), -9);
    ok = ok && tkz_encode_batch_packed_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, -3, ids.data(), cap, offs.data(), pos.data(), nullptr, 0, nullptr, &T, &rows, &segs) == TKZ_OK && pos == R.pos;
    if (ok && cap > 0) {
        T = rows = segs = -2;
        ok = tkz_encode_batch_packed_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, -3, ids.data(), cap - 1, offs.data(), pos.data(), seg.data(), nseg, nullptr, &T, &rows, &segs) == TKZ_E_CAPACITY;
        ok = ok && T == R.T && rows == R.n_rows && segs == nseg;
        ok = ok && tkz_encode_batch_packed_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, -3, ids.data(), cap, offs.data(), pos.data(), seg.data(), nseg - 1, nullptr, &T, &rows, &segs) == TKZ_E_CAPACITY;
        ok = ok && T == R.T && rows == R.n_rows && segs == nseg;
    }
    std::fill(ids.begin(), ids.end(), -9); std::fill(pos.begin(), pos.end(), -9); std::fill(seg.begin(), seg.end(), -9); std::fill(offs.begin(), offs.end(), -9);
    int64_t ni = -1, ns = -1;
    ok = ok && tkz_encode_batch_packed_utf8(e, d, b.offs.data(), n, nullptr, 0, bos, eos, L, -3, ids.data(), cap, offs.data(), pos.data(), seg.data(), nseg, &T, &ni, &ns) == TKZ_OK;
    ok = ok && T == R.T && ni == cap && ns == nseg && ids == R.ids && pos == R.pos && seg == R.seg && offs == R.offs;
    tkz_host_free(aligned);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string file = slurp(argv[1]);
    tkz_vocab* v = nullptr; tkz_encoder* e = nullptr;
    REQUIRE(tkz_vocab_from_tiktoken(reinterpret_cast<const uint8_t*>(file.data()), file.size(), &v) == TKZ_OK);
    REQUIRE(tkz_encoder_create(v, TKZ_PATTERN_CL100K, 0, &e) == TKZ_OK);
    const std::string eot = "<|endoftext|>";
    const int32_t sid[1] = {50256}; const int64_t loffs[2] = {0, (int64_t)eot.size()};
    REQUIRE(tkz_encoder_set_special_tokens(e, sid, reinterpret_cast<const uint8_t*>(eot.data()), loffs, 1) == TKZ_OK);
    const int32_t allow[1] = {0};
    const int32_t forms[4][2] = {{-1, -1}, {7, -1}, {-1, 9}, {7, 9}};
    for (int round = 0; round < 2; ++round) {
        {   // the framing forms over empty documents at the front, in runs of 1, 2 and 70, and at the end; every document empty; none
            Batch b; b.add(""); b.add(words(3)); b.add(""); b.add(words(5)); b.add(""); b.add(""); b.add(words(2)); for (int k = 0; k < 70; ++k) b.add(""); b.add(words(4)); b.add("");
            Batch empties; for (int k = 0; k < 5; ++k) empties.add("");
            Batch none;
            for (const auto& fr : forms) {
                for (int64_t L : {1, 4, 7}) REQUIRE(check_batch(e, b, L, fr[0], fr[1]));
                REQUIRE(check_batch(e, empties, 3, fr[0], fr[1]) && check_batch(e, none, 3, fr[0], fr[1]));
            }
        }
        {   // row lengths from 1 to ten times the stream
            Batch b; b.add(words(700)); b.add(""); b.add(words(1)); b.add(words(2300)); b.add(words(64)); b.add(""); b.add(words(1500));
            const int64_t T = 700 + 1 + 2300 + 64 + 1500 + 7;
            for (int64_t L : {int64_t(1), int64_t(2), int64_t(7), int64_t(64), int64_t(1000), K, 2 * K, T - 1, T, T + 1, 10 * T}) REQUIRE(check_batch(e, b, L, -1, 9));
            for (int64_t L : {int64_t(1), int64_t(7), K}) REQUIRE(check_batch(e, b, L, -1, -1));
        }
        {   // streams at the tile edges; a start at K and K - 1; three whole tiles; 300 documents in a tile; 300 empty documents between two tokens
            for (int64_t T : {K - 1, K, K + 1, 4 * K, 4 * K + 1}) {
                Batch b; b.add(words(100)); b.add(words(T - 107)); b.add(words(7));
                REQUIRE(check_batch(e, b, 512, -1, -1));
                Batch f; f.add(words(100)); f.add(words(T - 110)); f.add(words(7));
                REQUIRE(check_batch(e, f, 512, -1, 9));
            }
            for (int64_t first : {K - 1, K}) { Batch b; b.add(words(first)); b.add(words(10)); REQUIRE(check_batch(e, b, 3 * K, -1, -1) && check_batch(e, b, 3 * K, -1, 9)); }
            Batch three; three.add(words(10)); three.add(words(4 * K)); three.add(words(10));
            REQUIRE(check_batch(e, three, 1000, 7, 9));
            Batch many; for (int k = 0; k < 300; ++k) many.add(words(1));
            REQUIRE(check_batch(e, many, 50, -1, -1) && check_batch(e, many, 50, 7, 9));
            Batch gap; gap.add(words(5)); for (int k = 0; k < 300; ++k) gap.add(""); gap.add(words(5));
            REQUIRE(check_batch(e, gap, 4, -1, -1));
        }
        {   // a literal allowed, with eos set to the same id, and not allowed: against the special entry's ids
            const std::string text = words(3) + eot + words(9) + eot + eot;
            const int64_t offs[3] = {0, (int64_t)text.size(), (int64_t)text.size()};
            const uint8_t* t = reinterpret_cast<const uint8_t*>(text.data());
            for (int with = 0; with < 2; ++with) {
                std::vector<int32_t> want((size_t)text.size());
                std::vector<int64_t> wo(3);
                int64_t need = 0, T = 0, ni = 0, ns = 0;
                REQUIRE(tkz_encode_batch_special_utf8(e, t, offs, 2, allow, with, want.data(), (int64_t)want.size(), wo.data(), &need) == TKZ_OK);
                const Rows R = rule(want, wo, 5, -1, 50256, 0);
                std::vector<int32_t> ids(R.ids.size()), pos(R.ids.size());
                std::vector<int64_t> seg(R.seg.size()), oo(3);
                REQUIRE(tkz_encode_batch_packed_utf8(e, t, offs, 2, allow, with, -1, 50256, 5, 0, ids.data(), (int64_t)ids.size(), oo.data(), pos.data(), seg.data(), (int64_t)seg.size() - 1, &T, &ni, &ns) == TKZ_OK);
                REQUIRE(T == R.T && ids == R.ids && pos == R.pos && seg == R.seg && oo == R.offs && std::count(ids.begin(), ids.end(), 50256) == (with ? 5 : 2));
            }
        }
        {   // the UTF-16 entry: a lone surrogate, a pair cut by a document boundary, a literal; no units at all
            std::vector<uint16_t> u; std::vector<int64_t> uo{0};
            auto add = [&](const std::u16string& s) { u.insert(u.end(), s.begin(), s.end()); uo.push_back((int64_t)u.size()); };
            add(u"plain text"); add(u"lone \xD800 high zqxjkvb"); add(u"cut \xD83D"); add(u"\xDE00 here"); add(u""); add(u"a <|endoftext|> b \xD83D\xDE00\x6F22");
            const int64_t n = (int64_t)uo.size() - 1;
            std::vector<int32_t> want(u.size() * 3 + 1);
            std::vector<int64_t> wo((size_t)n + 1);
            int64_t need = 0, T = 0, ni = 0, ns = 0;
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), uo.data(), n, allow, 1, want.data(), (int64_t)want.size(), wo.data(), &need) == TKZ_OK);
            const Rows R = rule(want, wo, 6, 7, 9, -1);
            std::vector<int32_t> ids(R.ids.size()), pos(R.ids.size());
            std::vector<int64_t> seg(R.seg.size()), oo((size_t)n + 1);
            REQUIRE(tkz_encode_batch_packed_utf16(e, u.data(), uo.data(), n, allow, 1, 7, 9, 6, -1, ids.data(), (int64_t)ids.size() - 1, oo.data(), pos.data(), seg.data(), (int64_t)seg.size() - 1, &T, &ni, &ns) == TKZ_E_CAPACITY);
            REQUIRE(T == R.T && ni == (int64_t)R.ids.size() && ns == (int64_t)R.seg.size() - 1);
            REQUIRE(tkz_encode_batch_packed_utf16(e, u.data(), uo.data(), n, allow, 1, 7, 9, 6, -1, ids.data(), ni, oo.data(), pos.data(), seg.data(), ns, &T, &ni, &ns) == TKZ_OK);
            REQUIRE(ids == R.ids && pos == R.pos && seg == R.seg && oo == R.offs);
            const int64_t z[4] = {0, 0, 0, 0}; int32_t zi[8]; int32_t zp[8]; int64_t zs[8], zo[4];
            REQUIRE(tkz_encode_batch_packed_utf16(e, nullptr, z, 3, nullptr, 0, 7, 9, 4, 5, zi, 8, zo, zp, zs, 7, &T, &ni, &ns) == TKZ_OK && T == 6 && ni == 8 && ns == 3);
            REQUIRE(zi[0] == 7 && zi[1] == 9 && zi[5] == 9 && zi[6] == 5 && zi[7] == 5 && zo[3] == 6 && zs[0] == 0 && zs[1] == 2 && zs[2] == 4 && zs[3] == 6 && zp[1] == 1 && zp[4] == 0 && zp[7] == 0);
        }
        {   // the argument rows, invalid UTF-8
            const uint8_t t[5] = {'h', 'e', 0xFF, 'l', 'o'}; const int64_t o1[2] = {0, 2}, o2[2] = {0, 5}; int64_t oo[2], T = 7, ni = 7, ns = 7;
            int32_t ids[8], pos[8]; int64_t seg[9];
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, ids, 8, oo, pos, seg, 8, &T, &ni, &ns) == TKZ_OK && ni == 4 && ns == 1 && T >= 2 && T <= 3);
            REQUIRE(tkz_encode_batch_packed_utf8(nullptr, t, o1, 1, nullptr, 0, -1, 9, 4, 0, ids, 8, oo, pos, seg, 8, &T, &ni, &ns) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o1, 1, nullptr, 0, -2, 9, 4, 0, ids, 8, oo, pos, seg, 8, &T, &ni, &ns) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o1, 1, nullptr, 0, -1, -2, 4, 0, ids, 8, oo, pos, seg, 8, &T, &ni, &ns) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 0, 0, ids, 8, oo, pos, seg, 8, &T, &ni, &ns) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o1, 1, nullptr, 0, -1, 9, int64_t(1) << 31, 0, ids, 8, oo, pos, seg, 8, &T, &ni, &ns) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, ids, 8, nullptr, pos, seg, 8, &T, &ni, &ns) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, ids, 8, oo, pos, seg, -1, &T, &ni, &ns) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, ids, 8, oo, pos, seg, 8, &T, nullptr, &ns) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, ids, 8, oo, pos, seg, 8, nullptr, &ni, &ns) == TKZ_OK);
            REQUIRE(tkz_encode_batch_packed_device(e, t, o1, 1, 2, nullptr, 0, -1, 9, 4, 0, ids, 8, oo, pos, seg, 8, nullptr, nullptr, &ni, &ns) == TKZ_E_ARG);
            const int32_t bad[1] = {1}, twice[2] = {0, 0};
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o1, 1, bad, 1, -1, 9, 4, 0, ids, 8, oo, pos, seg, 8, &T, &ni, &ns) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o1, 1, twice, 2, -1, 9, 4, 0, ids, 8, oo, pos, seg, 8, &T, &ni, &ns) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_packed_utf8(e, t, o2, 1, nullptr, 0, -1, 9, 4, 0, ids, 8, oo, pos, seg, 8, &T, &ni, &ns) == TKZ_E_INVALID_UTF8);
        }
    }
    int64_t calls = 0;
    tkz_encoder_packed_calls(e, &calls);
    REQUIRE(calls > 100);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize packed ok (%lld packed calls)\n", (long long)calls);
    return 0;
}
