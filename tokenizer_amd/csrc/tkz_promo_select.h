// tkz_promo_select.h -- WHICH pieces a promotion adds (tkz_api.cpp: promote_from_memo), as a function of host copies alone: no device call, no lock.
#pragma once
#include <algorithm>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "tkz_kernels.h"
#include "tkz_vocab.h"

namespace tkz {

struct PromoSelection { int64_t added; uint32_t valid_slots; };     // pieces appended to the list; valid entries the memo held

// From the memo as read back, the sampled hit count of every slot (null: every valid entry counts alike) and the log of merged pieces of 17..28 bytes
// (kLongLogDwords dwords a record: 28 key bytes, len | count << 8, 4 tokens; may be empty), appends the new promoted pieces to items / keys / quads until the
// list holds `cap`: first the logged pieces seen at least twice -- real source text is full of them: "\n" + 19 spaces, by the hundred thousand --, up to a
// quarter of the cap, by count then key; then the valid memo entries by hits (stable: equal hits in slot order).  Never a key twice.
inline PromoSelection select_promotions(const std::vector<TkzMemoSlot>& memo, const std::vector<uint32_t>* hits, const std::vector<uint32_t>& llog, size_t cap,
                                        std::vector<KeyItem>* items, std::unordered_set<std::string>* keys, std::vector<uint32_t>* quads) {
    PromoSelection sel{0, 0};
    auto append = [&](const std::string& key, uint32_t cnt, const uint32_t* tokens) {
        items->push_back(KeyItem{key, kPromoFlag | ((cnt - 1u) << kPromoCntShift) | (uint32_t)items->size()});
        for (uint32_t t = 0; t < 4; ++t) quads->push_back(t < cnt ? (tokens[t] & 0x07FFFFFFu) : 0u);
        ++sel.added;
    };
    if (items->size() >= cap) return sel;
    if (!llog.empty()) {
        struct LongCand { uint32_t count; uint32_t rec; };
        std::unordered_map<std::string, LongCand> seen;
        for (size_t r = 0; r < llog.size() / kLongLogDwords; ++r) {
            const uint32_t* rec = &llog[r * kLongLogDwords];
            const uint32_t len = rec[7] & 0xFFu, cnt = (rec[7] >> 8) & 0xFFu;
            if (len <= 16 || len > (uint32_t)kLongLogMaxLen || cnt < 1 || cnt > 4) continue;
            std::string key(len, '\0');
            for (uint32_t b = 0; b < len; ++b) key[b] = (char)((rec[b >> 2] >> (8 * (b & 3))) & 0xFFu);
            auto it = seen.find(key);
            if (it == seen.end()) seen.emplace(key, LongCand{1u, (uint32_t)r}); else ++it->second.count;
        }
        std::vector<std::pair<uint32_t, const std::string*>> order;
        for (const auto& kv : seen) if (kv.second.count >= 2 && !keys->count(kv.first)) order.emplace_back(kv.second.count, &kv.first);
        std::sort(order.begin(), order.end(), [](const std::pair<uint32_t, const std::string*>& a, const std::pair<uint32_t, const std::string*>& b) { return a.first != b.first ? a.first > b.first : *a.second < *b.second; });
        const size_t long_room = std::min(cap - items->size(), std::max<size_t>(cap / 4, 1));
        for (size_t i = 0; i < order.size() && (size_t)sel.added < long_room; ++i) {
            const std::string& key = *order[i].second;
            const uint32_t* rec = &llog[(size_t)seen[key].rec * kLongLogDwords];
            keys->insert(key);
            append(key, (rec[7] >> 8) & 0xFFu, rec + 8);
        }
    }
    struct Cand { uint32_t hits, slot; };
    std::vector<Cand> cand;
    for (uint32_t i = 0; i < (uint32_t)memo.size(); ++i) {
        const uint32_t* v = memo[i].v;
        // the kernels' validity rule: the valid tag in every value word, not the BUSY mark; and a complete key: no zero byte inside its length, nothing
        // but zero bytes beyond it (other calls may be inserting while this copy was taken)
        if (!((v[0] & v[1] & v[2] & v[3]) & kMemoValid) || v[0] == kMemoBusy) continue;
        ++sel.valid_slots;
        if (hits && (*hits)[i] == 0) continue;
        const uint32_t len = ((v[1] >> 27) & 15u) + 1u;
        bool ok = true;
        for (uint32_t b = 0; b < 16 && ok; ++b) { const uint32_t byte = (memo[i].k[b >> 2] >> (8 * (b & 3))) & 0xFFu; ok = b < len ? byte != 0 : byte == 0; }
        if (!ok) continue;
        cand.push_back(Cand{hits ? (*hits)[i] : 1u, i});
    }
    std::stable_sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) { return a.hits > b.hits; });
    for (const Cand& c : cand) {
        if (items->size() >= cap) break;
        const TkzMemoSlot& m = memo[c.slot];
        const uint32_t len = ((m.v[1] >> 27) & 15u) + 1u, cnt = ((m.v[0] >> 29) & 3u) + 1u;
        std::string key(len, '\0');
        for (uint32_t b = 0; b < len; ++b) key[b] = (char)((m.k[b >> 2] >> (8 * (b & 3))) & 0xFFu);
        if (!keys->insert(key).second) continue;                        // (promoted before: a stale memo entry)
        append(key, cnt, m.v);
    }
    return sel;
}

}  // namespace tkz
