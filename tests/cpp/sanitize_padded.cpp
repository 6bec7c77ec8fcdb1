// A stand-alone driver for a sanitizer build of the host code behind the padded entries (tkz_encode_batch_padded_device / _utf8 / _utf16) and of k_pad_lens /
// k_pad_write: tests/test_cpp_padded.py compiles it with the product sources and the CPU SIMT emulator (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under
// -fsanitize=address,undefined and runs it; nothing is loaded into an interpreter.  It walks the shapes of tests/padded_cases.py -- the four framing forms over the
// cut edges on both cut and both pad sides, L == f and L == 1, the widths around a multiple and clamped, rows of 1 to 65 columns and across tiles, n_docs * W
// around a tile multiple, empty batches, a literal allowed and not, the UTF-16 entry with lone surrogates, the argument rows -- twice over one encoder, with
// buffers of EXACTLY n_docs * W, n_docs and n_docs + 1 entries (a store one past the end is the sanitizer's to find), one short of them, and without mask, pos and
// offsets.  Every result is held against the rule of tkz.h applied to the ids and offsets of the matching encode entry.  argv: gpt2.tiktoken
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

static const int64_t K = 1024;                               // kPadTile
static uint32_t g_rng = 2463534242u;
static uint32_t rnd(uint32_t n) { g_rng = g_rng * 1664525u + 1013904223u; return (g_rng >> 8) % n; }
static const char* kWords[] = {"the", "of", "and", "to", "in", "is", "that", "for", "it", "with", "as", "was", "on", "be", "at", "by", "this", "had", "not", "are"};
static std::string words(int64_t n) { std::string s; for (int64_t k = 0; k < n; ++k) { s += ' '; s += kWords[rnd(20)]; } return s; }      // n tokens

struct Batch { std::vector<uint8_t> bytes; std::vector<int64_t> offs{0}; void add(const std::string& d) { bytes.insert(bytes.end(), d.begin(), d.end()); offs.push_back((int64_t)bytes.size()); } };
struct Rows { int64_t total = 0, W = 0, n_cut = 0; std::vector<int32_t> ids, pos, lens; std::vector<uint8_t> mask; };

// the rule of tkz.h over the uncut ids and offsets
static Rows rule(const std::vector<int32_t>& ids, const std::vector<int64_t>& O, int64_t L, int32_t bos, int32_t eos, int32_t pad, int cut, int side, int64_t M) {
    Rows r;
    const int64_t n = (int64_t)O.size() - 1, fb = bos >= 0, fe = eos >= 0, f = fb + fe;
    r.total = O[(size_t)n];
    int64_t longest = 0;
    for (int64_t d = 0; d < n; ++d) {
        const int64_t nd = O[(size_t)d + 1] - O[(size_t)d], k = std::min<int64_t>(nd, L - f);
        r.lens.push_back((int32_t)(k + f));
        r.n_cut += nd > L - f;
        longest = std::max(longest, k + f);
    }
    r.W = longest == 0 ? 0 : (M == 0 ? L : std::min<int64_t>(L, (longest + M - 1) / M * M));
    r.ids.assign((size_t)(n * r.W), pad); r.pos.assign((size_t)(n * r.W), 0); r.mask.assign((size_t)(n * r.W), 0);
    for (int64_t d = 0; d < n; ++d) {
        const int64_t len = r.lens[(size_t)d], k = len - f, src = cut == TKZ_TRIM_SUFFIX ? O[(size_t)d] : O[(size_t)d + 1] - k;
        const int64_t s = d * r.W + (side == TKZ_PAD_LEFT ? r.W - len : 0);
        for (int64_t j = 0; j < len; ++j) {
            r.ids[(size_t)(s + j)] = fb && j == 0 ? bos : (fe && j == len - 1 ? eos : ids[(size_t)(src + j - fb)]);
            r.pos[(size_t)(s + j)] = (int32_t)j;
            r.mask[(size_t)(s + j)] = 1;
        }
    }
    return r;
}

// the device entry (the emulated build's device memory is host memory) with buffers of exactly n_docs * W, n_docs and n_docs + 1 entries; without the optional
// arrays; one entry short; the host entry
static bool check_batch(tkz_encoder* e, const Batch& b, int64_t L, int32_t bos, int32_t eos, int cut, int side, int64_t M) {
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
    const Rows R = rule(want_ids, want, L, bos, eos, -3, cut, side, M);
    const int64_t cap = n * R.W;
    std::vector<int32_t> ids((size_t)cap, -9), pos((size_t)cap, -9), lens((size_t)n, -9);
    std::vector<uint8_t> mask((size_t)cap, 9);
    std::vector<int64_t> offs((size_t)n + 1, -9);
    int32_t none = 0;                                                            // (an empty vector's data() may be null: the ids and lens pointers are required)
    int32_t* const pi = cap ? ids.data() : &none; int32_t* const pl = n ? lens.data() : &none;
    int64_t T = -1, W = -1, C = -1;
    ok = tkz_encode_batch_padded_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, cut, side, -3, M, pi, cap, mask.data(), pos.data(), pl, offs.data(), nullptr, &T, &W, &C) == TKZ_OK;
    ok = ok && T == R.total && W == R.W && C == R.n_cut && ids == R.ids && pos == R.pos && mask == R.mask && lens == R.lens && offs == want;
    std::fill(ids.begin(), ids.end(), -9); std::fill(lens.begin(), lens.end(), -9);
    ok = ok && tkz_encode_batch_padded_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, cut, side, -3, M, pi, cap, nullptr, nullptr, pl, nullptr, nullptr, &T, &W, &C) == TKZ_OK;
    ok = ok && ids == R.ids && lens == R.lens && W == R.W;
    std::fill(pos.begin(), pos.end(), -9);
    ok = ok && tkz_encode_batch_padded_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, cut, side, -3, M, pi, cap, nullptr, pos.data(), pl, nullptr, nullptr, &T, &W, &C) == TKZ_OK && pos == R.pos;
    if (ok && cap > 0) {
        T = W = C = -2;
        ok = tkz_encode_batch_padded_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, cut, side, -3, M, pi, cap - 1, mask.data(), pos.data(), pl, offs.data(), nullptr, &T, &W, &C) == TKZ_E_CAPACITY;
        ok = ok && T == R.total && W == R.W && C == R.n_cut;
    }
    std::fill(ids.begin(), ids.end(), -9); std::fill(pos.begin(), pos.end(), -9); std::fill(mask.begin(), mask.end(), 9); std::fill(lens.begin(), lens.end(), -9); std::fill(offs.begin(), offs.end(), -9);
    ok = ok && tkz_encode_batch_padded_utf8(e, d, b.offs.data(), n, nullptr, 0, bos, eos, L, cut, side, -3, M, pi, cap, mask.data(), pos.data(), pl, offs.data(), &T, &W, &C) == TKZ_OK;
    ok = ok && T == R.total && W == R.W && C == R.n_cut && ids == R.ids && pos == R.pos && mask == R.mask && lens == R.lens && offs == want;
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
        {   // the cut edges under the four framing forms, both cut sides, both pad sides; L == f; L == 1; empty batches
            const int64_t L = 9;
            Batch empties; for (int k = 0; k < 75; ++k) empties.add("");
            Batch none;
            for (const auto& fr : forms) {
                const int64_t f = (fr[0] >= 0) + (fr[1] >= 0);
                Batch b; for (int64_t n : {int64_t(0), int64_t(1), L - f - 1, L - f, L - f + 1, 3 * L}) b.add(words(n));
                for (int cut = 0; cut < 2; ++cut) for (int side = 0; side < 2; ++side) {
                    REQUIRE(check_batch(e, b, L, fr[0], fr[1], cut, side, 1));
                    if (f) REQUIRE(check_batch(e, b, f, fr[0], fr[1], cut, side, 1));
                    REQUIRE(check_batch(e, empties, 6, fr[0], fr[1], cut, side, side ? 0 : 8));
                }
                REQUIRE(check_batch(e, none, 3, fr[0], fr[1], 0, 0, 1));
            }
            Batch one; one.add(words(3)); one.add(""); one.add(words(1)); one.add(words(5));
            for (int cut = 0; cut < 2; ++cut) REQUIRE(check_batch(e, one, 1, -1, -1, cut, cut, 1));
        }
        {   // the width: the longest len a multiple of M, one below it and one above it; a round-up that exceeds L
            for (int64_t M : {int64_t(0), int64_t(1), int64_t(8), int64_t(64)}) {
                const int64_t base = std::max<int64_t>(M, 1) * (24 / std::max<int64_t>(M, 1) + 1);
                for (int64_t longest : {base - 1, base, base + 1}) {
                    Batch b; b.add(words(3)); b.add(words(longest - 1)); b.add(""); b.add(words(17));
                    REQUIRE(check_batch(e, b, 200, -1, 9, 0, 0, M) && check_batch(e, b, 200, -1, 9, 1, 1, M));
                }
            }
            Batch b; b.add(words(70)); b.add(words(5)); b.add(words(300));
            REQUIRE(check_batch(e, b, 100, 7, 9, 0, 0, 64) && check_batch(e, b, 21, 7, 9, 1, 1, 8) && check_batch(e, b, 63, 7, 9, 0, 1, 64) && check_batch(e, b, 7, 7, 9, 1, 0, 1000));
        }
        {   // rows of 1 to 65 columns (many rows in a group of 64 positions); a row across tiles; n_docs * W around a tile multiple
            for (int64_t W : {int64_t(1), int64_t(3), int64_t(7), int64_t(63), int64_t(64), int64_t(65)}) {
                Batch b; for (int64_t d = 0; d < 150; ++d) b.add(words((5 * d) % (W + 3)));
                REQUIRE(check_batch(e, b, W, -1, 9, 0, 0, 0) && check_batch(e, b, W, -1, 9, 1, 1, 0));
            }
            for (int64_t W : {K - 1, K, K + 1, 2 * K + 5}) {
                Batch b; b.add(words(W)); b.add(words(5)); b.add(words(W + 7));
                REQUIRE(check_batch(e, b, W, 7, -1, 0, 0, 1) && check_batch(e, b, W, 7, -1, 1, 1, 1));
            }
            const int64_t shapes[3][2] = {{23, 89}, {32, 64}, {3, 683}};            // 2K - 1, 2K, 2K + 1
            for (const auto& s : shapes) {
                Batch b; for (int64_t d = 0; d + 1 < s[0]; ++d) b.add(words((7 * d) % (s[1] + 2)));
                b.add(words(s[1]));
                REQUIRE(check_batch(e, b, s[1], -1, 9, 0, 0, 1) && check_batch(e, b, s[1], -1, 9, 0, 1, 1));
            }
        }
        {   // a literal allowed, with eos set to the same id, and not allowed: against the special entry's ids; the cut that removes it, and that keeps it last
            const std::string text = words(2) + eot + words(3);
            const std::string tail = words(3) + eot;
            const std::string both = text + tail;
            const int64_t offs[4] = {0, (int64_t)text.size(), (int64_t)both.size(), (int64_t)both.size()};
            const uint8_t* t = reinterpret_cast<const uint8_t*>(both.data());
            for (int with = 0; with < 2; ++with) {
                std::vector<int32_t> want((size_t)both.size());
                std::vector<int64_t> wo(4);
                int64_t need = 0;
                REQUIRE(tkz_encode_batch_special_utf8(e, t, offs, 3, allow, with, want.data(), (int64_t)want.size(), wo.data(), &need) == TKZ_OK);
                for (int64_t L : {int64_t(3), int64_t(4), int64_t(5), int64_t(8)}) for (int cut = 0; cut < 2; ++cut) {
                    const Rows R = rule(want, wo, L, -1, 50256, 0, cut, cut, 1);
                    std::vector<int32_t> ids(R.ids.size()), pos(R.ids.size()), lens(3);
                    std::vector<uint8_t> mask(R.ids.size());
                    std::vector<int64_t> oo(4);
                    int64_t T = 0, W = 0, C = 0;
                    REQUIRE(tkz_encode_batch_padded_utf8(e, t, offs, 3, allow, with, -1, 50256, L, cut, cut, 0, 1, ids.data(), (int64_t)ids.size(), mask.data(), pos.data(), lens.data(), oo.data(), &T, &W, &C) == TKZ_OK);
                    REQUIRE(T == R.total && W == R.W && C == R.n_cut && ids == R.ids && pos == R.pos && mask == R.mask && lens == R.lens && oo == wo);
                    if (with && L == 3 && cut == 0) REQUIRE(std::count(ids.begin(), ids.begin() + W, 50256) == 1);      // (the cut removed the literal: the eos alone)
                    if (with && L == 4 && cut == 0) REQUIRE(ids[2] == 50256 && ids[3] == 50256);                       // (the literal at the last kept position)
                }
            }
        }
        {   // the UTF-16 entry: a lone surrogate, a pair cut by a document boundary, a literal; no units at all
            std::vector<uint16_t> u; std::vector<int64_t> uo{0};
            auto add = [&](const std::u16string& s) { u.insert(u.end(), s.begin(), s.end()); uo.push_back((int64_t)u.size()); };
            add(u"plain text"); add(u"lone \xD800 high zqxjkvb"); add(u"cut \xD83D"); add(u"\xDE00 here"); add(u""); add(u"a <|endoftext|> b \xD83D\xDE00\x6F22");
            const int64_t n = (int64_t)uo.size() - 1;
            std::vector<int32_t> want(u.size() * 3 + 1);
            std::vector<int64_t> wo((size_t)n + 1);
            int64_t need = 0, T = 0, W = 0, C = 0;
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), uo.data(), n, allow, 1, want.data(), (int64_t)want.size(), wo.data(), &need) == TKZ_OK);
            const Rows R = rule(want, wo, 6, 7, 9, -1, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, 4);
            std::vector<int32_t> ids(R.ids.size()), pos(R.ids.size()), lens((size_t)n);
            std::vector<uint8_t> mask(R.ids.size());
            std::vector<int64_t> oo((size_t)n + 1);
            REQUIRE(tkz_encode_batch_padded_utf16(e, u.data(), uo.data(), n, allow, 1, 7, 9, 6, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, -1, 4, ids.data(), (int64_t)ids.size() - 1, mask.data(), pos.data(), lens.data(), oo.data(), &T, &W, &C) == TKZ_E_CAPACITY);
            REQUIRE(T == R.total && W == R.W && C == R.n_cut);
            REQUIRE(tkz_encode_batch_padded_utf16(e, u.data(), uo.data(), n, allow, 1, 7, 9, 6, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, -1, 4, ids.data(), n * W, mask.data(), pos.data(), lens.data(), oo.data(), &T, &W, &C) == TKZ_OK);
            REQUIRE(ids == R.ids && pos == R.pos && mask == R.mask && lens == R.lens && oo == wo);
            const int64_t z[4] = {0, 0, 0, 0}; int32_t zi[12]; int32_t zp[12]; uint8_t zm[12]; int32_t zl[3]; int64_t zo[4];
            REQUIRE(tkz_encode_batch_padded_utf16(e, nullptr, z, 3, nullptr, 0, 7, 9, 4, 0, 0, 5, 3, zi, 12, zm, zp, zl, zo, &T, &W, &C) == TKZ_OK && T == 0 && W == 3 && C == 0);
            REQUIRE(zi[0] == 7 && zi[1] == 9 && zi[2] == 5 && zi[8] == 5 && zm[1] == 1 && zm[2] == 0 && zp[1] == 1 && zp[2] == 0 && zl[2] == 2 && zo[3] == 0);
        }
        {   // the argument rows, invalid UTF-8
            const uint8_t t[5] = {'h', 'e', 0xFF, 'l', 'o'}; const int64_t o1[2] = {0, 2}, o2[2] = {0, 5}; int64_t oo[2], T = 7, W = 7, C = 7;
            int32_t ids[8], pos[8], lens[1]; uint8_t mask[8];
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_OK && W == lens[0] && T >= 1 && T <= 2 && C == 0);
            REQUIRE(tkz_encode_batch_padded_utf8(nullptr, t, o1, 1, nullptr, 0, -1, 9, 4, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -2, 9, 4, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, -2, 4, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 0, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, 7, 9, 1, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, 9, int64_t(1) << 31, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 2, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, -1, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, 0, 0, -1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, 0, 0, int64_t(1) << 31, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, 0, 0, 1, nullptr, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, 0, 0, 1, ids, 8, mask, pos, nullptr, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, nullptr, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, 0, 0, 1, ids, 8, nullptr, nullptr, lens, nullptr, &T, &W, &C) == TKZ_OK);
            REQUIRE(tkz_encode_batch_padded_device(e, t, o1, 1, 2, nullptr, 0, -1, 9, 4, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, nullptr, nullptr, &W, &C) == TKZ_E_ARG);
            const int32_t bad[1] = {1}, twice[2] = {0, 0};
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, bad, 1, -1, 9, 4, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o1, 1, twice, 2, -1, 9, 4, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_padded_utf8(e, t, o2, 1, nullptr, 0, -1, 9, 4, 0, 0, 0, 1, ids, 8, mask, pos, lens, oo, &T, &W, &C) == TKZ_E_INVALID_UTF8);
        }
    }
    int64_t calls = 0;
    tkz_encoder_padded_calls(e, &calls);
    REQUIRE(calls > 100);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize padded ok (%lld padded calls)\n", (long long)calls);
    return 0;
}
