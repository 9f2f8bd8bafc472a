// rcseg_fuzz.cpp — sanitizer harness for the segmented-stream host code (tic_rcseg_* in
// range_coder.cpp), built by `make asan-rcseg` with -fsanitize=address,undefined and run by
// tests/test_entropy_asan.py on the CPU.  A container is input a user hands in.
//
// Every buffer is a heap block of exactly the size passed, so a read or write one byte outside
// is a report.  Cases: round trips over random tables, counts and segment lengths, each segment
// compared with the file coder; random bytes, truncated, bit-flipped and length-inconsistent
// containers through parse and decode (rejected, or decoded to in-range symbols); containers
// with valid framing and random payloads (must decode, in range); every error path.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "tic.h"

static int g_fail = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                         \
    }                                                                   \
  } while (0)

// exact-size heap copy (std::vector may over-allocate)
struct Block {
  std::unique_ptr<uint8_t[]> p;
  size_t n = 0;
  explicit Block(size_t n_) : p(new uint8_t[n_ ? n_ : 1]), n(n_) {}
  Block(const uint8_t* src, size_t n_) : Block(n_) {
    if (n_) memcpy(p.get(), src, n_);
  }
};

static std::vector<int64_t> random_table(std::mt19937_64& g, int nsym, int64_t max_total) {
  std::vector<int64_t> cum(nsym + 1, 0);
  const int64_t top = std::max<int64_t>(1, std::min<int64_t>(2000, max_total / nsym - 1));
  for (int i = 0; i < nsym; ++i)
    cum[i + 1] = cum[i] + 1 + (int64_t)(g() % (uint64_t)(g() % 3 == 0 ? top : std::min<int64_t>(top, 20)));
  return cum;  // every frequency > 0, total <= max_total
}

static std::vector<uint8_t> encode_ok(const std::vector<uint8_t>& sym, uint32_t L, const std::vector<int64_t>& cum) {
  size_t cap = 0, w = 0;
  CHECK(tic_rcseg_bound(sym.size(), L, &cap) == TIC_OK);
  Block out(cap);
  Block in(sym.data(), sym.size());
  CHECK(tic_rcseg_encode(in.p.get(), in.n, L, cum.data(), cum.size(), out.p.get(), cap, &w) == TIC_OK);
  CHECK(w <= cap);
  return std::vector<uint8_t>(out.p.get(), out.p.get() + w);
}

// parse + decode of arbitrary bytes: either rejected, or n in-range symbols
static void try_decode(const std::vector<uint8_t>& bytes, const std::vector<int64_t>& cum, size_t n_hint) {
  Block b(bytes.data(), bytes.size());
  uint32_t L = 0;
  uint64_t n = 0;
  const int rc = tic_rcseg_parse(b.p.get(), b.n, &L, &n);
  CHECK(rc == TIC_OK || rc == TIC_EINVAL);
  if (rc != TIC_OK) {
    CHECK(strlen(tic_rc_last_error()) > 0);
    Block o(n_hint);
    CHECK(tic_rcseg_decode(b.p.get(), b.n, cum.data(), cum.size(), o.p.get(), n_hint) == TIC_EINVAL);
    return;
  }
  CHECK(n > 0);
  if (n > (1u << 22)) return;  // segments of length zero: many symbols from few bytes
  Block o((size_t)n);
  CHECK(tic_rcseg_decode(b.p.get(), b.n, cum.data(), cum.size(), o.p.get(), (size_t)n) == TIC_OK);
  for (size_t i = 0; i < n; ++i) CHECK(o.p[i] < cum.size() - 1);
  Block o2((size_t)n + 1);
  CHECK(tic_rcseg_decode(b.p.get(), b.n, cum.data(), cum.size(), o2.p.get(), (size_t)n + 1) == TIC_EINVAL);
}

int main(int argc, char** argv) {
  const char* dir = argc > 1 ? argv[1] : "/tmp";
  std::mt19937_64 g(20261020);
  const uint32_t Ls[] = {4, 8, 64, 1024, 4096, 16384};

  // --- round trips, each segment against the file coder ---
  for (int it = 0; it < 60; ++it) {
    const int nsym = 1 + (int)(g() % (it % 5 == 0 ? 256 : 6));
    const std::vector<int64_t> cum = random_table(g, nsym, it % 7 == 0 ? (1 << 24) : 70000);
    const uint32_t L = Ls[g() % 6];
    const size_t n = 1 + g() % (it % 4 == 0 ? 40000 : 300);
    std::vector<uint8_t> sym(n);
    for (auto& s : sym) s = (uint8_t)(g() % 11 == 0 ? g() % nsym : 0 + (g() % 2) * (nsym - 1));
    const std::vector<uint8_t> c = encode_ok(sym, L, cum);
    uint32_t pl = 0;
    uint64_t pn = 0;
    CHECK(tic_rcseg_parse(c.data(), c.size(), &pl, &pn) == TIC_OK && pl == L && pn == n);
    CHECK(tic_rcseg_parse(c.data(), c.size(), nullptr, nullptr) == TIC_OK);
    Block back(n);
    CHECK(tic_rcseg_decode(c.data(), c.size(), cum.data(), cum.size(), back.p.get(), n) == TIC_OK);
    CHECK(memcmp(back.p.get(), sym.data(), n) == 0);
    // segment payloads are the file coder's bytes
    const size_t S = (n + L - 1) / L;
    size_t at = 20 + 2 * S;
    for (size_t j = 0; j < S && j < 8; ++j) {
      const size_t len = c[20 + 2 * j] | (size_t)c[20 + 2 * j + 1] << 8;
      const size_t b = j * L, e = std::min(n, b + L);
      std::vector<int64_t> wide(sym.begin() + b, sym.begin() + e);
      const std::string path = std::string(dir) + "/rcseg_seg.bin";
      tic_rc_encoder* enc = nullptr;
      CHECK(tic_rc_encoder_open(path.c_str(), &enc) == TIC_OK);
      CHECK(tic_rc_encode(enc, wide.data(), wide.size(), cum.data(), cum.size()) == TIC_OK);
      CHECK(tic_rc_encoder_close(enc) == TIC_OK);
      tic_rc_encoder_free(enc);
      std::vector<uint8_t> fb;
      FILE* f = fopen(path.c_str(), "rb");
      int ch;
      while ((ch = fgetc(f)) != EOF) fb.push_back((uint8_t)ch);
      fclose(f);
      CHECK(fb.size() == len && (len == 0 || memcmp(fb.data(), c.data() + at, len) == 0));
      at += len;
    }

    // --- truncated, bit-flipped, extended ---
    for (int k = 0; k < 12; ++k) {
      std::vector<uint8_t> t(c.begin(), c.begin() + g() % (c.size() + 1));
      try_decode(t, cum, n);
      std::vector<uint8_t> fl = c;
      const size_t where = k < 6 ? g() % std::min<size_t>(fl.size(), 20 + 2 * S) : g() % fl.size();
      fl[where] ^= (uint8_t)(1u << (g() % 8));
      try_decode(fl, cum, n);
    }
    std::vector<uint8_t> ext = c;
    ext.push_back(0);
    try_decode(ext, cum, n);

    // --- inconsistent lengths: move a byte from one segment's length to another's, overflow one ---
    if (S >= 2) {
      std::vector<uint8_t> m = c;
      const size_t a = g() % S, b2 = (a + 1 + g() % (S - 1)) % S;
      auto rd = [&](size_t j) { return (uint32_t)(m[20 + 2 * j] | m[20 + 2 * j + 1] << 8); };
      auto wr = [&](size_t j, uint32_t v) {
        m[20 + 2 * j] = (uint8_t)v;
        m[20 + 2 * j + 1] = (uint8_t)(v >> 8);
      };
      if (rd(a) > 0) {
        wr(a, rd(a) - 1);
        wr(b2, rd(b2) + 1);
        try_decode(m, cum, n);  // still sums right: valid framing or a length above its limit
      }
      wr(a, 0xFFFF);
      try_decode(m, cum, n);
    }

    // --- valid framing, random payload: decodes, in range ---
    std::vector<uint8_t> rp = c;
    for (size_t i = 20 + 2 * S; i < rp.size(); ++i) rp[i] = (uint8_t)g();
    try_decode(rp, cum, n);
  }

  // --- random bytes behind a plausible header, and pure noise ---
  const std::vector<int64_t> cum2 = {0, 2457, 4096};
  for (int it = 0; it < 300; ++it) {
    std::vector<uint8_t> b(g() % 200);
    for (auto& v : b) v = (uint8_t)g();
    if (it % 2 == 0 && b.size() >= 20) {
      memcpy(b.data(), "TICS\x01\0\0\0", 8);
      const uint32_t L = it % 4 == 0 ? 4 * (1 + (uint32_t)(g() % 8)) : (uint32_t)g();
      memcpy(b.data() + 8, &L, 4);
      const uint64_t n = it % 8 < 6 ? g() % 100 : g();
      memcpy(b.data() + 12, &n, 8);
    }
    try_decode(b, cum2, 10);
  }
  try_decode({}, cum2, 1);

  // --- error paths ---
  {
    size_t cap = 0, w = 0;
    uint32_t L = 0;
    uint64_t n = 0;
    uint8_t sym[8] = {0, 1, 0, 1, 1, 0, 0, 2};
    uint8_t out[128];
    const int64_t cum[3] = {0, 3, 8};
    CHECK(tic_rcseg_bound(8, 4, nullptr) == TIC_EINVAL);
    CHECK(tic_rcseg_bound(0, 4, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound(8, 0, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound(8, 6, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound(8, 16388, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound(SIZE_MAX, 4, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound(8, 4, &cap) == TIC_OK && cap == 20 + 4 + 24 + 8);
    CHECK(tic_rcseg_encode(nullptr, 7, 4, cum, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode(sym, 7, 4, cum, 3, nullptr, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode(sym, 7, 4, cum, 3, out, sizeof(out), nullptr) == TIC_EINVAL);
    CHECK(tic_rcseg_encode(sym, 7, 4, nullptr, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode(sym, 7, 4, cum, 1, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode(sym, 0, 4, cum, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode(sym, 7, 5, cum, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode(sym, 8, 4, cum, 3, out, sizeof(out), &w) == TIC_EINVAL);  // symbol 2
    CHECK(strstr(tic_rc_last_error(), "outside the table") != nullptr);
    size_t need = 0;
    CHECK(tic_rcseg_bound(7, 4, &need) == TIC_OK);
    {
      Block o(need - 1);
      CHECK(tic_rcseg_encode(sym, 7, 4, cum, 3, o.p.get(), need - 1, &w) == TIC_EINVAL);
    }
    const int64_t zero_freq[4] = {0, 3, 3, 8}, big[3] = {0, 1, (int64_t)1 << 32}, wide[3] = {0, 1, (1 << 24) + 1};
    const int64_t down[3] = {0, 5, 4}, off[3] = {1, 2, 3};
    CHECK(tic_rcseg_encode(sym, 7, 4, zero_freq, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode(sym, 7, 4, big, 3, out, sizeof(out), &w) == TIC_EOVERFLOW);
    CHECK(tic_rcseg_encode(sym, 7, 4, wide, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode(sym, 7, 4, down, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode(sym, 7, 4, off, 3, out, sizeof(out), &w) == TIC_EINVAL);
    std::vector<int64_t> many(258);
    for (int i = 0; i < 258; ++i) many[i] = i;
    CHECK(tic_rcseg_encode(sym, 7, 4, many.data(), 258, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode(sym, 7, 4, many.data(), 257, out, sizeof(out), &w) == TIC_OK);
    CHECK(tic_rcseg_encode(sym, 7, 4, cum, 3, out, sizeof(out), &w) == TIC_OK && w > 24);
    CHECK(tic_rcseg_parse(nullptr, w, &L, &n) == TIC_EINVAL);
    CHECK(tic_rcseg_parse(out, w, &L, &n) == TIC_OK && L == 4 && n == 7);
    uint8_t back[8];
    CHECK(tic_rcseg_decode(out, w, cum, 3, nullptr, 7) == TIC_EINVAL);
    CHECK(tic_rcseg_decode(out, w, cum, 3, back, 6) == TIC_EINVAL);
    CHECK(tic_rcseg_decode(out, w, cum, 3, back, 8) == TIC_EINVAL);
    CHECK(tic_rcseg_decode(out, w, zero_freq, 4, back, 7) == TIC_EINVAL);
    CHECK(tic_rcseg_decode(out, w, many.data(), 258, back, 7) == TIC_EINVAL);
    CHECK(tic_rcseg_decode(out, w, big, 3, back, 7) == TIC_EOVERFLOW);
    CHECK(tic_rcseg_decode(out, w, cum, 3, back, 7) == TIC_OK && memcmp(back, sym, 7) == 0);
  }

  if (g_fail) {
    fprintf(stderr, "rcseg_fuzz: %d checks failed\n", g_fail);
    return 1;
  }
  printf("rcseg_fuzz ok\n");
  return 0;
}
