// Stand-alone check of the byte-level BPE tokenizer (bpe.cpp) for sanitizer builds: built with
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan
// from this file, bpe.cpp, wordpiece.cpp, unigram.cpp, fusion.cpp and host_stub.cpp (the last three: the shared helpers'
// and the stub's own dependencies), it has its own main, needs nothing preloaded, loads nothing into an
// interpreter and touches no GPU. Usage: bpe_check CASES, CASES a text file that tests/test_bpe_cpu.py writes from
// tests/golden/bpe_tokenizer.json (every string as hex of its bytes, "-" for the empty string):
//   P unk cls sep nfc | V n, n tokens | M n, n "left right" | A n, n "content id flags"
//   T n, n "max_len text n_ids ids..." | Q n, n "max_len a b seg_b n_ids ids..."
// It tokenises every recorded text and pair and compares the ids, then runs seeded random byte strings (malformed UTF-8
// among them, empty texts, max_len 2 and 3) through both calls, checking the short-buffer contract and the frame
// (cls first, sep last, at most max_len ids, seg_b inside the pair). Exit status 0: everything held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/voitta_engine.h"

static std::string unhex(const std::string& h) {
  std::string out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back(static_cast<char>(std::stoi(h.substr(i, 2), nullptr, 16)));
  return out;
}

static int fail(const char* what, long long i) {
  fprintf(stderr, "bpe_check: %s (case %lld): %s\n", what, i, vr_last_error());
  return 1;
}

static std::vector<const char*> ptrs(const std::vector<std::string>& v) {
  std::vector<const char*> p;
  for (const std::string& s : v) p.push_back(s.c_str());
  if (p.empty()) p.push_back("");
  return p;
}

static int encode_one(const vr_bpe* t, const std::string& s, int max_len, std::vector<int32_t>* ids) {
  const char* p = s.data();
  const int64_t len = static_cast<int64_t>(s.size());
  int64_t off[2], needed = 0;
  if (vr_bpe_encode(t, &p, &len, 1, max_len, off, nullptr, 0, &needed) != -2 || needed < 2 || needed > max_len) return 1;
  ids->assign(static_cast<size_t>(needed), -7);
  const int64_t asked = needed;
  if (vr_bpe_encode(t, &p, &len, 1, max_len, off, ids->data(), asked, &needed) != 0 || needed != asked || off[1] != asked)
    return 1;
  return 0;
}

static int encode_pair(const vr_bpe* t, const std::string& a, const std::string& b, int max_len, std::vector<int32_t>* ids,
                       int32_t* seg) {
  const char *pa = a.data(), *pb = b.data();
  const int64_t la = static_cast<int64_t>(a.size()), lb = static_cast<int64_t>(b.size());
  int64_t off[2], needed = 0;
  if (vr_bpe_encode_pairs(t, &pa, &la, &pb, &lb, 1, max_len, off, nullptr, seg, 0, &needed) != -2 || needed < 3 ||
      needed > max_len)
    return 1;
  ids->assign(static_cast<size_t>(needed), -7);
  const int64_t asked = needed;
  if (vr_bpe_encode_pairs(t, &pa, &la, &pb, &lb, 1, max_len, off, ids->data(), seg, asked, &needed) != 0 || needed != asked)
    return 1;
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return fail("usage: bpe_check CASES", 0);
  std::ifstream in(argv[1]);
  if (!in) return fail("cannot open the cases", 0);
  std::string tag;
  int unk = -1, cls = 0, sep = 0, nfc = 0;
  std::vector<std::string> vocab, ml, mr, added;
  std::vector<int32_t> added_ids, added_flags;
  vr_bpe* t = nullptr;
  long long checked = 0;
  while (in >> tag) {
    long long n = 0;
    if (tag == "P") {
      in >> unk >> cls >> sep >> nfc;
      continue;
    }
    in >> n;
    for (long long i = 0; i < n; ++i) {
      std::string a, b;
      if (tag == "V") {
        in >> a;
        vocab.push_back(unhex(a));
      } else if (tag == "M") {
        in >> a >> b;
        ml.push_back(unhex(a));
        mr.push_back(unhex(b));
      } else if (tag == "A") {
        int id, flags;
        in >> a >> id >> flags;
        added.push_back(unhex(a));
        added_ids.push_back(id);
        added_flags.push_back(flags);
      } else if (tag == "T" || tag == "Q") {
        if (!t) {
          const auto v = ptrs(vocab), l = ptrs(ml), r = ptrs(mr), ad = ptrs(added);
          if (vr_bpe_create(v.data(), static_cast<int32_t>(vocab.size()), l.data(), r.data(), static_cast<int32_t>(ml.size()),
                            unk, cls, sep, nfc, ad.data(), added_ids.data(), added_flags.data(),
                            static_cast<int32_t>(added.size()), &t) != 0)
            return fail("vr_bpe_create", 0);
        }
        int max_len, want_seg = 0;
        long long n_ids;
        in >> max_len >> a;
        if (tag == "Q") in >> b >> want_seg;
        in >> n_ids;
        std::vector<int32_t> want(static_cast<size_t>(n_ids)), got;
        for (int32_t& x : want) in >> x;
        int32_t seg = -1;
        if (tag == "T" ? encode_one(t, unhex(a), max_len, &got) : encode_pair(t, unhex(a), unhex(b), max_len, &got, &seg))
          return fail("encode", i);
        if (got != want || (tag == "Q" && seg != want_seg)) return fail("ids differ from the recorded ones", i);
        ++checked;
      } else {
        return fail("unknown section", i);
      }
    }
  }
  if (!t || checked == 0) return fail("no cases", 0);
  // seeded random byte strings: any bytes at all, biased towards UTF-8 lead and continuation bytes and white space
  std::mt19937 rng(12345);
  const unsigned char spice[] = {0x20, 0x20, 0x09, 0x0A, 0x27, 0x5B, 0x5D, 0xC3, 0xA9, 0xCC, 0x81, 0xE2, 0x80, 0x8D,
                                 0xF0, 0x9F, 0x91, 0x8D, 0xFF, 0xC0, 0xED, 0xA0, 0x80, 0xEA, 0xB0, 0x80, 0x00};
  auto text = [&] {
    std::string s;
    const int n = static_cast<int>(rng() % 48);
    for (int i = 0; i < n; ++i) {
      const unsigned r = rng();
      if (r % 7 == 0) s += "[MASK]";
      else if (r % 3 == 0) s.push_back(static_cast<char>(spice[(r >> 8) % sizeof(spice)]));
      else s.push_back(static_cast<char>((r >> 8) & 0xFF));
    }
    return s;
  };
  const int lens[] = {2, 3, 5, 16, 512};
  for (int it = 0; it < 3000; ++it) {
    const std::string a = it % 11 == 0 ? std::string() : text(), b = it % 13 == 0 ? std::string() : text();
    for (int max_len : lens) {
      std::vector<int32_t> ids;
      if (encode_one(t, a, max_len, &ids)) return fail("random text", it);
      if (ids.front() != cls || ids.back() != sep || static_cast<int>(ids.size()) > max_len) return fail("frame", it);
      if (max_len < 3) continue;
      int32_t seg = -1;
      if (encode_pair(t, a, b, max_len, &ids, &seg)) return fail("random pair", it);
      if (ids.front() != cls || ids.back() != sep || static_cast<int>(ids.size()) > max_len || seg < 2 ||
          seg >= static_cast<int>(ids.size()) || ids[static_cast<size_t>(seg) - 1] != sep)
        return fail("pair frame", it);
    }
  }
  vr_bpe_destroy(t);
  printf("bpe_check ok: %lld recorded cases, 3000 random texts and pairs\n", checked);
  return 0;
}
