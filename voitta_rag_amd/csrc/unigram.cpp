// SentencePiece Unigram tokenizer behind the C-ABI (vr_unigram_*): the tokenise step of the XLM-RoBERTa models
// (multilingual-e5, bge-reranker) as HF `tokenizers` runs it from their tokenizer.json. Host code, like wordpiece.cpp;
// batches run on the host threads.
//
// Pipeline, as the HF implementation (tokenizers 0.22) defines it:
//   added tokens   matched in the RAW text, leftmost-longest (aho-corasick LeftmostLongest); single_word keeps a match
//                  only between neighbours that are not word characters (\w); lstrip / rstrip widen it over White_Space (lstrip never
//                  past the previous match); the pieces between matches go through the rest separately
//   Precompiled    per extended grapheme cluster (UAX #29): a cluster under 6 bytes is looked up whole; otherwise, or
//                  when that misses, every code point is looked up alone and kept when it has no entry. A lookup is
//                  the darts-clone common-prefix search, and the FIRST (shortest) hit wins, as spm_precompiled does
//   Replace        " {2,}" -> " " (when the tokenizer.json has it)
//   pre-tokenise   Metaspace: ' ' -> U+2581, U+2581 prepended (always / on the piece that starts the text / never)
//                  unless already there, split before every U+2581; or WhitespaceSplit first (White_Space dropped),
//                  then Metaspace per word
//   Unigram        Viterbi over bytes with f64 scores and strict '>' (Unigram::encode_optimized); a character no
//                  piece covers is an unknown node of score min_score - 10; consecutive unknowns are fused into one
//                  string; every string is mapped back to its id (token_to_ids, a later duplicate winning), unk if none
//   post           <s> A </s>, <s> A </s> </s> B </s>; right truncation to max_len - 2, LongestFirst to max_len - 4
// One approximation: with prepend_scheme "first" after WhitespaceSplit, a word is taken to start the text when it
// is the first word of a piece that starts at byte 0 and nothing precedes it after normalisation (HF asks its byte
// alignments; the two differ only where the normaliser turns the text's first character into leading white space).
// Pinned against the HF `tokenizers` library on adversarial multilingual text (tests/test_unigram_cpu.py).

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "../../include/voitta_engine.h"
#include "engine_internal.h"
#include "grapheme_tables.inc"
#include "host_parallel.h"

namespace {

using u32s = std::u32string;

constexpr uint32_t kMeta = 0x2581;  // "▁"
constexpr double kUnkPenalty = 10.0;

// Grapheme_Cluster_Break classes as gen_grapheme_tables.py numbers them
enum Gcb : uint8_t { kOther, kCR, kLF, kControl, kExtend, kZWJ, kRI, kPrepend, kSpacingMark, kL, kV, kT, kLV, kLVT, kPict };

Gcb gcb_of(uint32_t c) {
  if (c >= 0x20 && c < 0x7F) return kOther;
  const size_t n = sizeof(kGcbRanges) / sizeof(kGcbRanges[0]);
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if (c < kGcbRanges[mid].lo) hi = mid;
    else if (c > kGcbRanges[mid].hi) lo = mid + 1;
    else return static_cast<Gcb>(kGcbRanges[mid].cls);
  }
  return kOther;
}

bool is_word_char(uint32_t c) {  // Unicode \w (the regex crate's is_word_character)
  if (c < 128) return (c >= '0' && c <= '9') || ((c | 32) >= 'a' && (c | 32) <= 'z') || c == '_';
  const size_t n = sizeof(kWordCharRanges) / sizeof(kWordCharRanges[0]);
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if (c < kWordCharRanges[mid][0]) hi = mid;
    else if (c > kWordCharRanges[mid][1]) lo = mid + 1;
    else return true;
  }
  return false;
}

// end of the extended grapheme cluster that starts at t[i] (UAX #29 GB3-GB13; GB9c's Indic conjuncts are not joined:
// their clusters are at least 9 bytes, past the whole-cluster lookup, so they are looked up per code point either way)
size_t cluster_end(const u32s& t, size_t i, size_t n) {
  Gcb prev = gcb_of(t[i]);
  int pict = prev == kPict ? 1 : 0;  // 1: ExtPict Extend*, 2: ExtPict Extend* ZWJ
  int ri = prev == kRI ? 1 : 0;
  size_t j = i + 1;
  for (; j < n; ++j) {
    const Gcb cur = gcb_of(t[j]);
    bool brk;
    if (prev == kCR && cur == kLF) brk = false;
    else if (prev == kCR || prev == kLF || prev == kControl) brk = true;
    else if (cur == kCR || cur == kLF || cur == kControl) brk = true;
    else if (prev == kL && (cur == kL || cur == kV || cur == kLV || cur == kLVT)) brk = false;
    else if ((prev == kLV || prev == kV) && (cur == kV || cur == kT)) brk = false;
    else if ((prev == kLVT || prev == kT) && cur == kT) brk = false;
    else if (cur == kExtend || cur == kZWJ || cur == kSpacingMark || prev == kPrepend) brk = false;
    else if (prev == kZWJ && cur == kPict && pict == 2) brk = false;
    else if (prev == kRI && cur == kRI && (ri & 1)) brk = false;
    else brk = true;
    if (brk) break;
    pict = cur == kPict ? 1 : (cur == kExtend && pict == 1) ? 1 : (cur == kZWJ && pict == 1) ? 2 : 0;
    ri = cur == kRI ? ri + 1 : 0;
    prev = cur;
  }
  return j;
}

// A byte trie over the pieces for the Viterbi's common-prefix search: the children of a node are contiguous and
// sorted by byte.
struct ByteTrie {
  struct Node {
    uint32_t first = 0;  // first child
    uint16_t count = 0;  // children
    uint8_t byte = 0;
    int32_t value = -1;  // piece id ending here
  };
  std::vector<Node> nodes;

  void build(const std::vector<std::pair<std::string, int32_t>>& keys) {  // sorted, distinct, non-empty
    nodes.assign(1, Node());
    struct Span { uint32_t node; size_t lo, hi, depth; };
    std::vector<Span> todo{{0, 0, keys.size(), 0}};
    for (size_t q = 0; q < todo.size(); ++q) {
      const Span s = todo[q];
      size_t lo = s.lo;
      if (lo < s.hi && keys[lo].first.size() == s.depth) nodes[s.node].value = keys[lo++].second;
      const uint32_t first = static_cast<uint32_t>(nodes.size());
      uint16_t count = 0;
      for (size_t a = lo; a < s.hi;) {
        const unsigned char b = static_cast<unsigned char>(keys[a].first[s.depth]);
        size_t z = a + 1;
        while (z < s.hi && static_cast<unsigned char>(keys[z].first[s.depth]) == b) ++z;
        Node c;
        c.byte = b;
        nodes.push_back(c);
        todo.push_back({first + count, a, z, s.depth + 1});
        ++count;
        a = z;
      }
      nodes[s.node].first = first;
      nodes[s.node].count = count;
    }
  }
  int32_t child(int32_t node, unsigned char b) const {
    const Node& n = nodes[static_cast<size_t>(node)];
    uint32_t lo = n.first, hi = n.first + n.count;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) / 2;
      if (nodes[mid].byte < b) lo = mid + 1;
      else hi = mid;
    }
    return lo < n.first + n.count && nodes[lo].byte == b ? static_cast<int32_t>(lo) : -1;
  }
};

struct Added {
  u32s content;
  int32_t id;
  int32_t flags;
};

}  // namespace

struct vr_unigram final : vr::Tokenizer {
  std::vector<double> scores;
  std::unordered_map<std::string, int32_t> to_id;  // HF token_to_ids: a later duplicate overwrites an earlier one
  ByteTrie trie;
  double unk_score = 0;
  int32_t unk = -1, bos = -1, eos = -1;
  std::vector<uint32_t> darts;  // the charsmap's double array (empty: no Precompiled normalizer)
  std::string replacements;     // ... and its NUL-separated replacement strings
  bool replace_spaces = false;
  int32_t pre = VR_UNIGRAM_PRE_METASPACE, prepend = VR_PREPEND_ALWAYS;
  std::vector<Added> added;

  int encode(const char* const* texts, const int64_t* text_lens, int64_t n_texts, int32_t max_len, int64_t* out_offsets,
             int32_t* out_ids, int64_t capacity, int64_t* needed) const override {
    return vr_unigram_encode(this, texts, text_lens, n_texts, max_len, out_offsets, out_ids, capacity, needed);
  }
  int encode_pairs(const char* const* a_texts, const int64_t* a_lens, const char* const* b_texts, const int64_t* b_lens,
                   int64_t n, int32_t max_len, int64_t* out_offsets, int32_t* out_ids, int32_t* out_seg_b,
                   int64_t capacity, int64_t* needed) const override {
    return vr_unigram_encode_pairs(this, a_texts, a_lens, b_texts, b_lens, n, max_len, out_offsets, out_ids, out_seg_b,
                                   capacity, needed);
  }
};

namespace {

// spm_precompiled's transform: the replacement of the shortest key that is a prefix of s, or nullptr
const char* charsmap_lookup(const vr_unigram& t, const std::string& s) {
  const std::vector<uint32_t>& a = t.darts;
  auto offset = [](uint32_t u) { return static_cast<size_t>((u >> 10) << ((u & (1u << 9)) >> 6)); };
  size_t pos = 0;
  pos ^= offset(a[0]);
  for (unsigned char c : s) {
    if (c == 0) break;
    pos ^= c;
    if (pos >= a.size()) return nullptr;
    const uint32_t unit = a[pos];
    if ((unit & ((1u << 31) | 0xFFu)) != c) return nullptr;
    pos ^= offset(unit);
    if (pos >= a.size()) return nullptr;
    if ((unit >> 8) & 1u) {
      const size_t v = a[pos] & ((1u << 31) - 1);
      return v < t.replacements.size() ? t.replacements.c_str() + v : nullptr;
    }
  }
  return nullptr;
}

void append_replacement(const char* r, u32s* out) {
  u32s cps;
  vr::decode_utf8(r, strlen(r), &cps);
  out->append(cps);
}

// Precompiled, then Replace(" {2,}", " ")
void normalize(const vr_unigram& t, const char32_t* in, size_t n, u32s* out) {
  out->clear();
  if (t.darts.empty()) {
    out->assign(in, n);
  } else {
    const u32s text(in, n);
    std::string buf;
    for (size_t i = 0; i < n;) {
      const size_t j = cluster_end(text, i, n);
      buf.clear();
      for (size_t k = i; k < j; ++k) vr::append_utf8(text[k], &buf);
      const char* r = buf.size() < 6 ? charsmap_lookup(t, buf) : nullptr;
      if (r) {
        append_replacement(r, out);
      } else {
        for (size_t k = i; k < j; ++k) {
          buf.clear();
          vr::append_utf8(text[k], &buf);
          const char* rc = charsmap_lookup(t, buf);
          if (rc) append_replacement(rc, out);
          else out->push_back(text[k]);
        }
      }
      i = j;
    }
  }
  if (t.replace_spaces) {  // a ' ' that follows a ' ' goes
    size_t w = 0;
    bool after_space = false;
    for (size_t r = 0; r < out->size(); ++r) {
      const uint32_t c = (*out)[r];
      if (!(c == ' ' && after_space)) (*out)[w++] = c;
      after_space = c == ' ';
    }
    out->resize(w);
  }
}

// Unigram::encode_optimized over one pre-tokenised word (UTF-8 bytes), ids appended
void viterbi(const vr_unigram& t, const std::string& w, std::vector<int32_t>* ids) {
  struct Best { double score; int32_t start; int32_t id; };
  const size_t n = w.size();
  std::vector<Best> best(n + 1, Best{0.0, -1, 0});
  for (size_t s = 0; s < n;) {
    const double here = best[s].score;
    const unsigned char lead = static_cast<unsigned char>(w[s]);
    const size_t mblen = std::min(n - s, static_cast<size_t>(lead < 0x80 ? 1 : lead < 0xE0 ? 2 : lead < 0xF0 ? 3 : 4));
    bool single = false;
    int32_t node = 0;
    for (size_t e = s; e < n; ++e) {
      node = t.trie.child(node, static_cast<unsigned char>(w[e]));
      if (node < 0) break;
      const int32_t id = t.trie.nodes[static_cast<size_t>(node)].value;
      if (id < 0) continue;
      Best& b = best[e + 1];
      const double cand = t.scores[static_cast<size_t>(id)] + here;
      if (b.start < 0 || cand > b.score) b = Best{cand, static_cast<int32_t>(s), id};
      if (e + 1 - s == mblen) single = true;
    }
    if (!single) {
      Best& b = best[s + mblen];
      const double cand = t.unk_score + here;
      if (b.start < 0 || cand > b.score) b = Best{cand, static_cast<int32_t>(s), t.unk};
    }
    s += mblen;
  }
  // back from the end; runs of unknowns fuse into one string
  std::vector<std::pair<size_t, size_t>> spans;  // reversed
  size_t end = n, unk_end = 0;
  bool in_unk = false;
  while (end > 0) {
    const Best& b = best[end];
    const size_t start = static_cast<size_t>(b.start);
    if (b.id == t.unk) {
      if (!in_unk) unk_end = end;
      in_unk = true;
    } else {
      if (in_unk) spans.emplace_back(end, unk_end);
      in_unk = false;
      spans.emplace_back(start, end);
    }
    end = start;
  }
  if (in_unk) spans.emplace_back(0, unk_end);
  for (size_t k = spans.size(); k-- > 0;) {
    auto it = t.to_id.find(w.substr(spans[k].first, spans[k].second - spans[k].first));
    ids->push_back(it == t.to_id.end() ? t.unk : it->second);
  }
}

// one pre-tokenised word of the normalised text: Metaspace (prepend, split before every U+2581), then the Viterbi
void metaspace_word(const vr_unigram& t, const char32_t* w, size_t n, bool starts_text, std::vector<int32_t>* ids,
                    std::string* buf) {
  u32s m;
  m.reserve(n + 1);
  const bool add = n > 0 && w[0] != kMeta && w[0] != ' ' &&
                   (t.prepend == VR_PREPEND_ALWAYS || (t.prepend == VR_PREPEND_FIRST && starts_text));
  if (add) m.push_back(kMeta);
  for (size_t i = 0; i < n; ++i) m.push_back(w[i] == ' ' ? kMeta : w[i]);
  size_t a = 0;
  while (a < m.size()) {
    size_t b = a + 1;
    while (b < m.size() && m[b] != kMeta) ++b;
    buf->clear();
    for (size_t k = a; k < b; ++k) vr::append_utf8(m[k], buf);
    viterbi(t, *buf, ids);
    a = b;
  }
}

// the ids of one text (no specials), appended to *ids until it holds `cap` or more
void pieces(const vr_unigram& t, const char* s, size_t n, size_t cap, std::vector<int32_t>* ids) {
  u32s raw, norm;
  vr::decode_utf8(s, n, &raw);
  const size_t len = raw.size();
  std::string buf;
  // a stretch of raw text between added tokens: normalise, pre-tokenise, Viterbi
  auto stretch = [&](size_t a, size_t b) {
    if (a >= b) return;
    normalize(t, raw.data() + a, b - a, &norm);
    if (t.pre == VR_UNIGRAM_PRE_METASPACE) {
      metaspace_word(t, norm.data(), norm.size(), a == 0, ids, &buf);
      return;
    }
    for (size_t i = 0; i < norm.size() && ids->size() < cap;) {
      if (vr::is_white_space(norm[i])) {
        ++i;
        continue;
      }
      size_t j = i;
      while (j < norm.size() && !vr::is_white_space(norm[j])) ++j;
      metaspace_word(t, norm.data() + i, j - i, a == 0 && i == 0, ids, &buf);
      i = j;
    }
  };
  size_t done = 0;  // end of the last match (HF's start_offset)
  for (size_t i = 0; i < len && ids->size() < cap;) {
    const Added* hit = nullptr;
    for (const Added& ad : t.added)
      if (ad.content.size() <= len - i && (!hit || ad.content.size() > hit->content.size()) &&
          std::equal(ad.content.begin(), ad.content.end(), raw.begin() + static_cast<std::ptrdiff_t>(i)))
        hit = &ad;
    if (!hit) {
      ++i;
      continue;
    }
    size_t start = i, stop = i + hit->content.size();
    i = stop;  // the search goes on after the match itself, whatever the stripping takes
    if ((hit->flags & VR_ADDED_SINGLE_WORD) &&
        ((start > 0 && is_word_char(raw[start - 1])) || (stop < len && is_word_char(raw[stop]))))
      continue;
    if (hit->flags & VR_ADDED_LSTRIP) {
      size_t ns = start;
      while (ns > 0 && vr::is_white_space(raw[ns - 1])) --ns;
      start = std::max(ns, done);
    }
    if (hit->flags & VR_ADDED_RSTRIP)
      while (stop < len && vr::is_white_space(raw[stop])) ++stop;
    stretch(done, start);
    if (ids->size() < cap) ids->push_back(hit->id);
    done = stop;
  }
  if (ids->size() < cap) stretch(done, len);
}

void encode_one(const vr_unigram& t, const char* s, size_t n, int32_t max_len, std::vector<int32_t>* ids) {
  ids->clear();
  if (t.bos >= 0) ids->push_back(t.bos);  // (the template $A </s> of a T5 tokenizer has no <s>)
  const size_t budget = static_cast<size_t>(max_len) - 1;  // ids before </s>
  pieces(t, s, n, budget + 64, ids);  // (+64: a word may add several pieces; trimmed below)
  if (ids->size() > budget) ids->resize(budget);
  ids->push_back(t.eos);
}

}  // namespace

namespace vr {
const Tokenizer* as_tokenizer(const vr_unigram* t) { return t; }
bool is_word_character(uint32_t c) { return is_word_char(c); }
}  // namespace vr

extern "C" {

int vr_unigram_create(const char* const* pieces_in, const double* scores, int32_t n_pieces, int32_t unk_id, int32_t bos_id,
                      int32_t eos_id, const uint8_t* charsmap, int64_t charsmap_len, int32_t replace_spaces,
                      int32_t pre_tokenizer, int32_t prepend_scheme, const char* const* added, const int32_t* added_ids,
                      const int32_t* added_flags, int32_t n_added, vr_unigram** out) {
  VR_CHECK(pieces_in && scores && out && n_pieces > 0 && n_added >= 0 && charsmap_len >= 0, "bad arguments");
  VR_CHECK(n_added == 0 || (added && added_ids && added_flags), "bad added-token arguments");
  VR_CHECK(charsmap_len == 0 || charsmap, "null charsmap");
  auto valid_id = [&](int32_t i) { return i >= 0 && i < n_pieces; };
  // bos_id -1: the template is $A </s> (T5), not <s> $A </s>
  VR_CHECK(valid_id(unk_id) && (bos_id == -1 || valid_id(bos_id)) && valid_id(eos_id), "unk / bos / eos id outside the %d pieces",
           n_pieces);
  VR_CHECK(pre_tokenizer == VR_UNIGRAM_PRE_METASPACE || pre_tokenizer == VR_UNIGRAM_PRE_WHITESPACE_METASPACE,
           "unknown pre-tokenizer %d", pre_tokenizer);
  VR_CHECK(prepend_scheme >= VR_PREPEND_ALWAYS && prepend_scheme <= VR_PREPEND_NEVER, "unknown prepend scheme %d",
           prepend_scheme);
  vr_unigram* t = new vr_unigram();
  std::unique_ptr<vr_unigram> guard(t);
  t->scores.assign(scores, scores + n_pieces);
  double min_score = 1e300;
  t->to_id.reserve(static_cast<size_t>(n_pieces) * 2);
  for (int32_t i = 0; i < n_pieces; ++i) {
    VR_CHECK(pieces_in[i], "piece %d is null", i);
    t->to_id[pieces_in[i]] = i;
    min_score = std::min(min_score, scores[i]);
  }
  t->unk_score = min_score - kUnkPenalty;
  {
    std::vector<std::pair<std::string, int32_t>> keys;
    keys.reserve(t->to_id.size());
    for (const auto& kv : t->to_id)
      if (!kv.first.empty()) keys.emplace_back(kv.first, kv.second);
    std::sort(keys.begin(), keys.end());
    t->trie.build(keys);
  }
  t->unk = unk_id;
  t->bos = bos_id;
  t->eos = eos_id;
  if (charsmap_len > 0) {
    // spm_precompiled: u32 trie size in bytes, the double array, then the replacement strings
    VR_CHECK(charsmap_len >= 4, "charsmap of %lld bytes", static_cast<long long>(charsmap_len));
    uint32_t trie_bytes = 0;
    memcpy(&trie_bytes, charsmap, 4);
    const uint64_t units = trie_bytes / 4;
    VR_CHECK(units >= 1 && 4 + units * 4 <= static_cast<uint64_t>(charsmap_len), "charsmap trie of %u bytes in %lld",
             trie_bytes, static_cast<long long>(charsmap_len));
    t->darts.resize(units);
    memcpy(t->darts.data(), charsmap + 4, units * 4);
    t->replacements.assign(reinterpret_cast<const char*>(charsmap) + 4 + units * 4,
                           static_cast<size_t>(charsmap_len - 4 - static_cast<int64_t>(units) * 4));
  }
  t->replace_spaces = replace_spaces != 0;
  t->pre = pre_tokenizer;
  t->prepend = prepend_scheme;
  for (int32_t i = 0; i < n_added; ++i) {
    VR_CHECK(added[i] && added[i][0], "added token %d is empty", i);
    VR_CHECK(added_ids[i] >= 0, "added token %d has id %d", i, added_ids[i]);
    VR_CHECK((added_flags[i] & ~(VR_ADDED_LSTRIP | VR_ADDED_RSTRIP | VR_ADDED_SINGLE_WORD)) == 0,
             "added token %d: unknown flags %d", i, added_flags[i]);
    Added a;
    vr::decode_utf8(added[i], strlen(added[i]), &a.content);
    a.id = added_ids[i];
    a.flags = added_flags[i];
    t->added.push_back(std::move(a));
  }
  *out = guard.release();
  return 0;
}

void vr_unigram_destroy(vr_unigram* t) { delete t; }

int vr_unigram_encode(const vr_unigram* t, const char* const* texts, const int64_t* text_lens, int64_t n_texts,
                      int32_t max_len, int64_t* out_offsets, int32_t* out_ids, int64_t capacity, int64_t* needed) {
  VR_CHECK(t && n_texts >= 0 && (n_texts == 0 || (texts && text_lens)) && out_offsets && needed, "bad arguments");
  VR_CHECK(max_len >= 2, "max_len %d cannot hold <s> and </s>", max_len);
  for (int64_t i = 0; i < n_texts; ++i)
    VR_CHECK(texts[i] && text_lens[i] >= 0, "text %lld: null or negative length", static_cast<long long>(i));
  std::vector<std::vector<int32_t>> per_text(static_cast<size_t>(n_texts));
  vr::parallel_for(n_texts, 16, [&](int64_t i) {
    encode_one(*t, texts[i], static_cast<size_t>(text_lens[i]), max_len, &per_text[static_cast<size_t>(i)]);
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

int vr_unigram_encode_pairs(const vr_unigram* t, const char* const* a_texts, const int64_t* a_lens,
                            const char* const* b_texts, const int64_t* b_lens, int64_t n, int32_t max_len,
                            int64_t* out_offsets, int32_t* out_ids, int32_t* out_seg_b, int64_t capacity,
                            int64_t* needed) {
  VR_CHECK(t && n >= 0 && (n == 0 || (a_texts && a_lens && b_texts && b_lens)) && out_offsets && needed, "bad arguments");
  VR_CHECK(t->bos >= 0, "this tokenizer's template is $A </s>: it has no pair template (<s> $A </s> </s> $B </s>)");
  VR_CHECK(max_len >= 4, "max_len %d cannot hold <s> and three </s>", max_len);
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
  const size_t m = static_cast<size_t>(max_len) - 4;
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
    total += static_cast<int64_t>(na + nb + 4);
    out_offsets[i + 1] = total;
    if (out_seg_b) out_seg_b[i] = static_cast<int32_t>(na + 3);
  }
  if (out_ids && total <= capacity)
    vr::parallel_for(n, 256, [&](int64_t i) {
      const std::vector<int32_t>& a = a_ids[static_cast<size_t>(a_of[static_cast<size_t>(i)])];
      const std::vector<int32_t>& b = b_ids[static_cast<size_t>(i)];
      const size_t na = keep_a[static_cast<size_t>(i)], nb = keep_b[static_cast<size_t>(i)];
      int32_t* o = out_ids + out_offsets[i];
      *o++ = t->bos;
      std::copy(a.begin(), a.begin() + static_cast<std::ptrdiff_t>(na), o);
      o += na;
      *o++ = t->eos;
      *o++ = t->eos;
      std::copy(b.begin(), b.begin() + static_cast<std::ptrdiff_t>(nb), o);
      o += nb;
      *o = t->eos;
    });
  *needed = total;
  if (total > capacity) {
    vr::set_error("output buffer holds %lld ids, %lld needed", static_cast<long long>(capacity), static_cast<long long>(total));
    return -2;  // offsets, seg_b and *needed are valid: call again with a larger buffer
  }
  return 0;
}

}  // extern "C"
