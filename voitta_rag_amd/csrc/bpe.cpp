// Byte-level BPE tokenizer (vr_bpe_*): the tokenise step of the ModernBERT models (gte-modernbert-base,
// modernbert-embed-base, gte-reranker-modernbert-base) as HF `tokenizers` runs it from their tokenizer.json. Host code,
// like wordpiece.cpp and unigram.cpp; the steps and their order are in include/voitta_engine.h. Every other pipeline is
// refused on the Python side (voitta_rag_amd/bpe.py), which then falls back to the library.
//
// The GPT-2 split is a hand-written scanner over code points (no regex engine): at each position the alternatives of
//   's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+
// are tried in that order, each greedy, as a backtracking regex does. \p{L} and \p{N} come from bpe_tables.inc, \s is
// Unicode White_Space. The look-ahead of \s+(?!\S) gives a white-space run that reaches the end of the text whole, and
// any other run without its last character — which the following alternative of the next piece picks up (" word").
//
// BPE of a piece follows the library's Word::merge_all: the symbols are a linked list, every adjacent pair that is a
// merge sits in a priority queue ordered by (rank, position), and a popped entry is applied only if both symbols still
// are what they were — n log n in the piece's length. No memo of pieces is kept: the object is read-only.

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <queue>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "../../include/voitta_engine.h"
#include "engine_internal.h"
#include "bpe_tables.inc"
#include "host_parallel.h"

namespace {

using u32s = std::u32string;

template <size_t N>
bool in_ranges(const uint32_t (&r)[N][2], uint32_t cp) {
  size_t lo = 0, hi = N;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if (cp < r[mid][0]) hi = mid;
    else if (cp > r[mid][1]) lo = mid + 1;
    else return true;
  }
  return false;
}

inline bool is_letter(uint32_t c) {
  if (c < 128) return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z');
  return in_ranges(kLetterRanges, c);
}
inline bool is_number(uint32_t c) {
  if (c < 128) return c >= '0' && c <= '9';
  return in_ranges(kNumberRanges, c);
}
using vr::is_white_space;
inline bool is_other(uint32_t c) { return !is_white_space(c) && !is_letter(c) && !is_number(c); }

// the primary composite of (a, b), or 0: Hangul L + V and LV + T algorithmically, the rest from kCompose
uint32_t compose(uint32_t a, uint32_t b) {
  if (a >= 0x1100 && a < 0x1113 && b >= 0x1161 && b < 0x1176) return 0xAC00 + ((a - 0x1100) * 21 + (b - 0x1161)) * 28;
  if (a >= 0xAC00 && a <= 0xD7A3 && (a - 0xAC00) % 28 == 0 && b > 0x11A7 && b < 0x11C3) return a + (b - 0x11A7);
  const size_t n = sizeof(kCompose) / sizeof(kCompose[0]);
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if (kCompose[mid].first < a || (kCompose[mid].first == a && kCompose[mid].second < b)) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && kCompose[lo].first == a && kCompose[lo].second == b ? kCompose[lo].composite : 0;
}

// NFC: NFD (decomposition and canonical reordering, wordpiece.cpp), then canonical composition: a character combines
// with the last starter unless a character between them blocks it (one of combining class 0, or of a class not below
// its own)
void nfc(const u32s& in, u32s* out) {
  bool ascii = true;
  for (char32_t c : in) ascii = ascii && c < 0xC0;
  if (ascii) {  // (nothing below U+00C0 decomposes or combines)
    *out = in;
    return;
  }
  u32s d;
  vr::nfd_text(in, &d);
  out->clear();
  ptrdiff_t starter = -1;
  uint32_t last_cc = 0;
  for (char32_t c : d) {
    const uint32_t cc = vr::combining_class(c);
    if (starter >= 0) {
      const bool adjacent = static_cast<ptrdiff_t>(out->size()) - 1 == starter;
      if (adjacent || last_cc < cc) {
        const uint32_t both = compose((*out)[static_cast<size_t>(starter)], c);
        if (both) {
          (*out)[static_cast<size_t>(starter)] = both;
          continue;
        }
      }
    }
    if (cc == 0) starter = static_cast<ptrdiff_t>(out->size());
    last_cc = cc;
    out->push_back(c);
  }
}

struct Added {
  u32s content;
  int32_t id;
  int32_t flags;
};

struct PairHash {
  size_t operator()(uint64_t k) const { return static_cast<size_t>(k * 0x9E3779B97F4A7C15ull >> 17); }
};

}  // namespace

struct vr_bpe final : vr::Tokenizer {
  std::unordered_map<std::string, int32_t> to_id;
  int32_t byte_id[256];  // the id of each byte's one-character token, or -1
  std::unordered_map<uint64_t, std::pair<int32_t, int32_t>, PairHash> merges;  // (left id, right id) -> (rank, new id)
  int32_t unk = -1, cls = -1, sep = -1;
  bool nfc = false;
  std::vector<Added> raw_added, norm_added;  // matched before / after the normaliser

  int encode(const char* const* texts, const int64_t* text_lens, int64_t n_texts, int32_t max_len, int64_t* out_offsets,
             int32_t* out_ids, int64_t capacity, int64_t* needed) const override {
    return vr_bpe_encode(this, texts, text_lens, n_texts, max_len, out_offsets, out_ids, capacity, needed);
  }
  int encode_pairs(const char* const* a_texts, const int64_t* a_lens, const char* const* b_texts, const int64_t* b_lens,
                   int64_t n, int32_t max_len, int64_t* out_offsets, int32_t* out_ids, int32_t* out_seg_b,
                   int64_t capacity, int64_t* needed) const override {
    return vr_bpe_encode_pairs(this, a_texts, a_lens, b_texts, b_lens, n, max_len, out_offsets, out_ids, out_seg_b,
                               capacity, needed);
  }
};

namespace {

inline uint64_t pair_key(int32_t a, int32_t b) {
  return (static_cast<uint64_t>(static_cast<uint32_t>(a)) << 32) | static_cast<uint32_t>(b);
}

// GPT-2's byte -> code point map: the printable Latin-1 bytes stand for themselves, the others are U+0100 + k in byte order
uint32_t byte_char(int b) {
  static const std::vector<uint32_t> table = [] {
    std::vector<uint32_t> t(256);
    int k = 0;
    for (int i = 0; i < 256; ++i) {
      const bool keep = (i >= 0x21 && i <= 0x7E) || (i >= 0xA1 && i <= 0xAC) || (i >= 0xAE && i <= 0xFF);
      t[static_cast<size_t>(i)] = keep ? static_cast<uint32_t>(i) : 0x100u + static_cast<uint32_t>(k++);
    }
    return t;
  }();
  return table[static_cast<size_t>(b)];
}

struct Symbol {
  int32_t id, prev, next;
  bool live;
};
struct Candidate {
  int32_t rank, pos, new_id;
  bool operator<(const Candidate& o) const { return rank != o.rank ? rank > o.rank : pos > o.pos; }  // (a max-heap)
};

// BPE of one pre-token (its UTF-8 bytes), the ids appended to *ids
void bpe_piece(const vr_bpe& t, const std::string& bytes, std::vector<Symbol>* syms, std::vector<int32_t>* ids) {
  syms->clear();
  for (unsigned char b : bytes) {
    int32_t id = t.byte_id[b];
    if (id < 0) {
      if (t.unk < 0) continue;  // no unk token: the library drops the symbol
      id = t.unk;
    }
    const int32_t k = static_cast<int32_t>(syms->size());
    syms->push_back({id, k - 1, -1, true});
    if (k > 0) (*syms)[static_cast<size_t>(k) - 1].next = k;
  }
  std::vector<Symbol>& s = *syms;
  std::priority_queue<Candidate> queue;
  auto offer = [&](int32_t pos) {
    const int32_t nx = s[static_cast<size_t>(pos)].next;
    if (nx < 0) return;
    const auto it = t.merges.find(pair_key(s[static_cast<size_t>(pos)].id, s[static_cast<size_t>(nx)].id));
    if (it != t.merges.end()) queue.push({it->second.first, pos, it->second.second});
  };
  for (int32_t i = 0; i + 1 < static_cast<int32_t>(s.size()); ++i) offer(i);
  while (!queue.empty()) {
    const Candidate top = queue.top();
    queue.pop();
    Symbol& left = s[static_cast<size_t>(top.pos)];
    if (!left.live || left.next < 0) continue;
    Symbol& right = s[static_cast<size_t>(left.next)];
    const auto it = t.merges.find(pair_key(left.id, right.id));
    if (it == t.merges.end() || it->second.second != top.new_id) continue;  // the pair is no longer what was queued
    left.id = top.new_id;
    right.live = false;
    left.next = right.next;
    if (right.next >= 0) s[static_cast<size_t>(right.next)].prev = top.pos;
    if (left.prev >= 0) offer(left.prev);
    offer(top.pos);
  }
  for (const Symbol& y : s)
    if (y.live) ids->push_back(y.id);
}

// the end of the GPT-2 piece that starts at i (i < n)
size_t split_end(const char32_t* x, size_t i, size_t n) {
  if (x[i] == U'\'' && i + 1 < n) {
    const char32_t a = x[i + 1], b = i + 2 < n ? x[i + 2] : 0;
    if (a == U's' || a == U't') return i + 2;
    if ((a == U'r' && b == U'e') || (a == U'v' && b == U'e')) return i + 3;
    if (a == U'm') return i + 2;
    if (a == U'l' && b == U'l') return i + 3;
    if (a == U'd') return i + 2;
  }
  const bool space = x[i] == U' ' && i + 1 < n;  // the optional space; without it x[i] itself must be of the class
  for (int kind = 0; kind < 3; ++kind) {
    auto is = [&](uint32_t c) { return kind == 0 ? is_letter(c) : kind == 1 ? is_number(c) : is_other(c); };
    size_t e = space && is(x[i + 1]) ? i + 2 : is(x[i]) ? i + 1 : 0;
    if (e == 0) continue;
    while (e < n && is(x[e])) ++e;
    return e;
  }
  // white space: the whole run at the end of the text, else the run without its last character, else (one character
  // in front of a word) that character
  size_t e = i;
  while (e < n && is_white_space(x[e])) ++e;
  if (e == n || e - i == 1) return e;
  return e - 1;
}

// a stretch of normalised text without added tokens: split, bytes, BPE
void plain(const vr_bpe& t, const char32_t* x, size_t n, size_t cap, std::vector<int32_t>* ids, std::string* buf,
           std::vector<Symbol>* syms) {
  for (size_t i = 0; i < n && ids->size() < cap;) {
    const size_t e = split_end(x, i, n);
    buf->clear();
    for (size_t k = i; k < e; ++k) vr::append_utf8(x[k], buf);
    bpe_piece(t, *buf, syms, ids);
    i = e;
  }
}

// `text` cut at the tokens of `added` (leftmost, the longest at a position; lstrip / rstrip / single_word as HF honours
// them): between(a, b) for the stretches, token(id) for the matches, in order
template <class Between, class Token>
void cut(const std::vector<Added>& added, const u32s& text, Between between, Token token) {
  const size_t len = text.size();
  size_t done = 0;
  if (!added.empty())
    for (size_t i = 0; i < len;) {
      const Added* hit = nullptr;
      for (const Added& ad : added)
        if (ad.content.size() <= len - i && (!hit || ad.content.size() > hit->content.size()) &&
            std::equal(ad.content.begin(), ad.content.end(), text.begin() + static_cast<std::ptrdiff_t>(i)))
          hit = &ad;
      if (!hit) {
        ++i;
        continue;
      }
      size_t start = i, stop = i + hit->content.size();
      i = stop;
      if ((hit->flags & VR_ADDED_SINGLE_WORD) &&
          ((start > 0 && vr::is_word_character(text[start - 1])) || (stop < len && vr::is_word_character(text[stop]))))
        continue;
      if (hit->flags & VR_ADDED_LSTRIP) {
        size_t ns = start;
        while (ns > 0 && is_white_space(text[ns - 1])) --ns;
        start = std::max(ns, done);
      }
      if (hit->flags & VR_ADDED_RSTRIP)
        while (stop < len && is_white_space(text[stop])) ++stop;
      if (start > done) between(done, start);
      token(hit->id);
      done = stop;
    }
  if (len > done) between(done, len);
}

// the ids of one text (no specials), appended to *ids until it holds `cap` or more
void pieces(const vr_bpe& t, const char* s, size_t n, size_t cap, std::vector<int32_t>* ids) {
  u32s raw, part, norm;
  vr::decode_utf8(s, n, &raw);
  std::string buf;
  std::vector<Symbol> syms;
  cut(t.raw_added, raw,
      [&](size_t a, size_t b) {
        if (ids->size() >= cap) return;
        part.assign(raw, a, b - a);
        if (t.nfc) nfc(part, &norm);
        else norm = part;
        cut(t.norm_added, norm,
            [&](size_t c, size_t d) { plain(t, norm.data() + c, d - c, cap, ids, &buf, &syms); },
            [&](int32_t id) {
              if (ids->size() < cap) ids->push_back(id);
            });
      },
      [&](int32_t id) {
        if (ids->size() < cap) ids->push_back(id);
      });
}

}  // namespace

namespace vr {
const Tokenizer* as_tokenizer(const vr_bpe* t) { return t; }
}  // namespace vr

extern "C" {

int vr_bpe_create(const char* const* vocab, int32_t n_vocab, const char* const* merge_left, const char* const* merge_right,
                  int32_t n_merges, int32_t unk_id, int32_t cls_id, int32_t sep_id, int32_t nfc_on, const char* const* added,
                  const int32_t* added_ids, const int32_t* added_flags, int32_t n_added, vr_bpe** out) {
  VR_CHECK(vocab && out && n_vocab > 0 && n_merges >= 0 && n_added >= 0, "bad arguments");
  VR_CHECK(n_merges == 0 || (merge_left && merge_right), "null merges");
  VR_CHECK(n_added == 0 || (added && added_ids && added_flags), "bad added-token arguments");
  auto valid_id = [&](int32_t i) { return i >= 0 && i < n_vocab; };
  VR_CHECK(unk_id == -1 || valid_id(unk_id), "unk id %d outside the %d tokens (-1: none)", unk_id, n_vocab);
  VR_CHECK(valid_id(cls_id) && valid_id(sep_id), "cls / sep id outside the %d tokens", n_vocab);
  vr_bpe* t = new vr_bpe();
  std::unique_ptr<vr_bpe> guard(t);
  t->to_id.reserve(static_cast<size_t>(n_vocab) * 2);
  for (int32_t i = 0; i < n_vocab; ++i) {
    VR_CHECK(vocab[i], "token %d is null", i);
    t->to_id[vocab[i]] = i;
  }
  for (int b = 0; b < 256; ++b) {
    std::string key;
    vr::append_utf8(byte_char(b), &key);
    const auto it = t->to_id.find(key);
    t->byte_id[b] = it == t->to_id.end() ? -1 : it->second;
  }
  t->merges.reserve(static_cast<size_t>(n_merges) * 2);
  for (int32_t r = 0; r < n_merges; ++r) {
    VR_CHECK(merge_left[r] && merge_right[r], "merge %d is null", r);
    const auto a = t->to_id.find(merge_left[r]), b = t->to_id.find(merge_right[r]);
    const auto both = t->to_id.find(std::string(merge_left[r]) + merge_right[r]);
    VR_CHECK(a != t->to_id.end() && b != t->to_id.end() && both != t->to_id.end(),
             "merge %d: '%s' + '%s' or their concatenation is not in the vocabulary", r, merge_left[r], merge_right[r]);
    t->merges.emplace(pair_key(a->second, b->second), std::make_pair(r, both->second));  // (the first of duplicates holds)
  }
  t->unk = unk_id;
  t->cls = cls_id;
  t->sep = sep_id;
  t->nfc = nfc_on != 0;
  for (int32_t i = 0; i < n_added; ++i) {
    VR_CHECK(added[i] && added[i][0], "added token %d is empty", i);
    VR_CHECK(added_ids[i] >= 0, "added token %d has id %d", i, added_ids[i]);
    VR_CHECK((added_flags[i] & ~(VR_ADDED_LSTRIP | VR_ADDED_RSTRIP | VR_ADDED_SINGLE_WORD | VR_ADDED_NORMALIZED)) == 0,
             "added token %d: unknown flags %d", i, added_flags[i]);
    Added a;
    vr::decode_utf8(added[i], strlen(added[i]), &a.content);
    a.id = added_ids[i];
    a.flags = added_flags[i];
    if (a.flags & VR_ADDED_NORMALIZED) {  // (the library normalises such a token's content as it does the text)
      if (t->nfc) {
        u32s n;
        nfc(a.content, &n);
        a.content = n;
      }
      t->norm_added.push_back(std::move(a));
    } else {
      t->raw_added.push_back(std::move(a));
    }
  }
  *out = guard.release();
  return 0;
}

void vr_bpe_destroy(vr_bpe* t) { delete t; }

int vr_bpe_encode(const vr_bpe* t, const char* const* texts, const int64_t* text_lens, int64_t n_texts, int32_t max_len,
                  int64_t* out_offsets, int32_t* out_ids, int64_t capacity, int64_t* needed) {
  VR_CHECK(t && n_texts >= 0 && (n_texts == 0 || (texts && text_lens)) && out_offsets && needed, "bad arguments");
  VR_CHECK(max_len >= 2, "max_len %d cannot hold the two special tokens", max_len);
  for (int64_t i = 0; i < n_texts; ++i)
    VR_CHECK(texts[i] && text_lens[i] >= 0, "text %lld: null or negative length", static_cast<long long>(i));
  std::vector<std::vector<int32_t>> per_text(static_cast<size_t>(n_texts));
  vr::parallel_for(n_texts, 16, [&](int64_t i) {
    std::vector<int32_t>& ids = per_text[static_cast<size_t>(i)];
    const size_t budget = static_cast<size_t>(max_len) - 1;  // ids before sep
    ids.push_back(t->cls);
    pieces(*t, texts[i], static_cast<size_t>(text_lens[i]), budget, &ids);
    if (ids.size() > budget) ids.resize(budget);
    ids.push_back(t->sep);
  });
  int64_t total = 0;
  out_offsets[0] = 0;
  for (int64_t i = 0; i < n_texts; ++i) {
    total += static_cast<int64_t>(per_text[static_cast<size_t>(i)].size());
    out_offsets[i + 1] = total;
  }
  if (out_ids && total <= capacity)
    vr::parallel_for(n_texts, 256, [&](int64_t i) {
      const std::vector<int32_t>& ids = per_text[static_cast<size_t>(i)];
      memcpy(out_ids + out_offsets[i], ids.data(), ids.size() * sizeof(int32_t));
    });
  *needed = total;
  if (total > capacity) {
    vr::set_error("output buffer holds %lld ids, %lld needed", static_cast<long long>(capacity), static_cast<long long>(total));
    return -2;  // offsets and *needed are valid: call again with a larger buffer
  }
  return 0;
}

int vr_bpe_encode_pairs(const vr_bpe* t, const char* const* a_texts, const int64_t* a_lens, const char* const* b_texts,
                        const int64_t* b_lens, int64_t n, int32_t max_len, int64_t* out_offsets, int32_t* out_ids,
                        int32_t* out_seg_b, int64_t capacity, int64_t* needed) {
  VR_CHECK(t && n >= 0 && (n == 0 || (a_texts && a_lens && b_texts && b_lens)) && out_offsets && needed, "bad arguments");
  VR_CHECK(max_len >= 3, "max_len %d cannot hold the three special tokens of a pair", max_len);
  for (int64_t i = 0; i < n; ++i)
    VR_CHECK(a_texts[i] && b_texts[i] && a_lens[i] >= 0 && b_lens[i] >= 0, "pair %lld: null text or negative length",
             static_cast<long long>(i));
  // every distinct A text once (a question is paired with each of its candidates)
  std::unordered_map<std::string_view, int64_t> first;
  std::vector<int64_t> a_of(static_cast<size_t>(n));
  std::vector<int64_t> uniq;
  for (int64_t i = 0; i < n; ++i) {
    auto it = first.emplace(std::string_view(a_texts[i], static_cast<size_t>(a_lens[i])), static_cast<int64_t>(uniq.size()));
    if (it.second) uniq.push_back(i);
    a_of[static_cast<size_t>(i)] = it.first->second;
  }
  // both sides in full: where the truncation splits depends on both untruncated lengths
  const size_t m = static_cast<size_t>(max_len) - 3;
  std::vector<std::vector<int32_t>> a_ids(uniq.size()), b_ids(static_cast<size_t>(n));
  vr::parallel_for(static_cast<int64_t>(uniq.size()), 4, [&](int64_t u) {
    const int64_t i = uniq[static_cast<size_t>(u)];
    pieces(*t, a_texts[i], static_cast<size_t>(a_lens[i]), SIZE_MAX, &a_ids[static_cast<size_t>(u)]);
  });
  vr::parallel_for(n, 4, [&](int64_t i) {
    pieces(*t, b_texts[i], static_cast<size_t>(b_lens[i]), SIZE_MAX, &b_ids[static_cast<size_t>(i)]);
  });
  std::vector<size_t> keep_a(static_cast<size_t>(n)), keep_b(static_cast<size_t>(n));
  int64_t total = 0;
  out_offsets[0] = 0;
  for (int64_t i = 0; i < n; ++i) {
    size_t na = a_ids[static_cast<size_t>(a_of[static_cast<size_t>(i)])].size(), nb = b_ids[static_cast<size_t>(i)].size();
    vr::longest_first(&na, &nb, m);
    keep_a[static_cast<size_t>(i)] = na;
    keep_b[static_cast<size_t>(i)] = nb;
    total += static_cast<int64_t>(na + nb + 3);
    out_offsets[i + 1] = total;
    if (out_seg_b) out_seg_b[i] = static_cast<int32_t>(na + 2);
  }
  if (out_ids && total <= capacity)
    vr::parallel_for(n, 256, [&](int64_t i) {
      const std::vector<int32_t>& a = a_ids[static_cast<size_t>(a_of[static_cast<size_t>(i)])];
      const std::vector<int32_t>& b = b_ids[static_cast<size_t>(i)];
      const size_t na = keep_a[static_cast<size_t>(i)], nb = keep_b[static_cast<size_t>(i)];
      int32_t* o = out_ids + out_offsets[i];
      *o++ = t->cls;
      std::copy(a.begin(), a.begin() + static_cast<std::ptrdiff_t>(na), o);
      o += na;
      *o++ = t->sep;
      std::copy(b.begin(), b.begin() + static_cast<std::ptrdiff_t>(nb), o);
      o += nb;
      *o = t->sep;
    });
  *needed = total;
  if (total > capacity) {
    vr::set_error("output buffer holds %lld ids, %lld needed", static_cast<long long>(capacity), static_cast<long long>(total));
    return -2;  // offsets, seg_b and *needed are valid: call again with a larger buffer
  }
  return 0;
}

}  // extern "C"
