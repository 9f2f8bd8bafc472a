// range_coder.cpp — static-model range coder behind the C-ABI (include/tic.h, tic_rc_*).
//
// Replaces the third-party `range_coder` extension the reference imports
// (encode.py:9,76-97; decode.py:9,79-101): RangeEncoder(path).encode(symbols, cum_freq),
// RangeDecoder(path).decode(n, cum_freq), with the same argument contract and error
// classes as its test-suite pins (other/test_range_coder.py:13-136).  The package itself
// is not vendored, so its byte format is not reproduced bit for bit.
//
// Coder: 32-bit range with exact arithmetic — `range` starts at 2^32 (held in 64 bits),
// so power-of-two totals subdivide it without rounding; `low` is kept in 64 bits and a
// carry is resolved with a cached byte + a count of pending 0xFF bytes.  A byte leaves
// the coder whenever range < 2^24.  close() flushes the FEWEST bytes k (0..4) whose
// zero-extension lies in [low, low + range), so a stream of b information bits costs
// ceil(b/8) bytes when the model is dyadic: the KAT input (cum_freq [0,4,6,8],
// [0,0,0,0,1,2] x 17 = 136 bits) encodes to exactly 17 bytes of 0x0b.
// The decoder reads zeros past the end of the file.  Several encode() calls (each with
// its own table) append to one stream and are decoded by matching decode() calls.
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tic.h"

namespace {
thread_local std::string g_rc_err;
int rc_fail(int code, const std::string& m) {
  g_rc_err = m;
  return code;
}

constexpr uint64_t kTop = 1ull << 24;
constexpr uint64_t kFull = 1ull << 32;
constexpr int64_t kMaxTotal = 1ll << 24;  // range >= 2^24 after normalisation

// Validate a cumulative frequency table (the reference's ValueError / OverflowError
// contract: other/test_range_coder.py:13-34,70-88,122-128).
int check_table(const int64_t* cum, size_t ncum, int64_t* total) {
  if (!cum || ncum < 2) return rc_fail(TIC_EINVAL, "invalid frequency table (needs >= 2 entries)");
  for (size_t i = 0; i < ncum; ++i)
    if (cum[i] < 0 || cum[i] >= (int64_t)kFull)
      return rc_fail(TIC_EOVERFLOW, "cumulative frequencies must fit in an unsigned 32-bit integer");
  if (cum[0] != 0) return rc_fail(TIC_EINVAL, "cumulative frequency table must start at 0");
  for (size_t i = 1; i < ncum; ++i)
    if (cum[i] < cum[i - 1]) return rc_fail(TIC_EINVAL, "cumulative frequencies must be non-decreasing");
  if (cum[ncum - 1] <= 0) return rc_fail(TIC_EINVAL, "invalid frequency table (zero total)");
  if (cum[ncum - 1] > kMaxTotal) return rc_fail(TIC_EINVAL, "total frequency must be <= 2^24");
  *total = cum[ncum - 1];
  return TIC_OK;
}

// The coder core, over any byte sink / source: the file API below and the segmented container
// (tic_rcseg_*) run the same arithmetic, so a segment's payload is the file's bytes.
template <class Sink>
struct EncCore {
  Sink s;
  uint64_t low = 0, range = kFull;
  int cache = -1;          // byte waiting for a possible carry (-1: none yet)
  uint64_t pending = 0;    // 0xFF bytes after the cache

  bool put(int b) { return s.put(b); }
  bool emit_top() {  // move the top byte of the 32-bit window (bits 24..31) out of low
    if (low < 0xFF000000ull || low >= kFull) {
      const int carry = low >= kFull ? 1 : 0;
      if (cache >= 0 && !put((cache + carry) & 0xFF)) return false;
      for (; pending; --pending)
        if (!put((0xFF + carry) & 0xFF)) return false;
      cache = (int)((low >> 24) & 0xFF);
    } else {
      ++pending;  // top byte is 0xFF and a carry may still arrive
    }
    low = (low << 8) & (kFull - 1);
    return true;
  }
  // one symbol [start, start + freq) of `total`; last: start + freq == total
  bool symbol(uint64_t start, uint64_t freq, uint64_t total, bool last) {
    const uint64_t r = range / total;
    low += start * r;
    range = last ? range - start * r : freq * r;
    while (range < kTop) {
      range <<= 8;
      if (!emit_top()) return false;
    }
    return true;
  }
  // the minimal flush: fewest top bytes k of a value v in [low, low + range) whose remaining
  // bytes are zero
  bool finish() {
    int k = 0;
    uint64_t v = low;
    for (; k <= 4; ++k) {
      const int shift = 32 - 8 * k;
      const uint64_t unit = shift >= 64 ? 0 : (1ull << shift);
      v = k == 4 ? low : ((low + unit - 1) / unit) * unit;
      if (v < low + range) break;
    }
    bool ok = true;
    low = v;
    for (int i = 0; i < k && ok; ++i) ok = emit_top();
    if (ok && k > 0) {  // drain cache + pending (with the carry already folded in)
      if (cache >= 0) ok = put(cache);
      for (; ok && pending; --pending) ok = put(0xFF);
    } else if (ok && cache >= 0) {
      const int carry = v >= kFull ? 1 : 0;
      ok = put((cache + carry) & 0xFF);
      for (; ok && pending; --pending) ok = put((0xFF + carry) & 0xFF);
    }
    return ok;
  }
};

template <class Source>
struct DecCore {
  Source s;
  uint64_t code = 0, range = kFull;
  void start() {
    for (int i = 0; i < 4; ++i) code = (code << 8) | (uint64_t)s.get();
  }
  int64_t symbol(const int64_t* cum, int64_t nsym, uint64_t total) {
    const uint64_t r = range / total;
    uint64_t val = code / r;
    if (val >= total) val = total - 1;
    // last s with cum[s] <= val (and freq > 0)
    int64_t lo = 0, hi = nsym - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) / 2;
      if ((uint64_t)cum[mid] <= val) lo = mid;
      else hi = mid - 1;
    }
    const uint64_t start = (uint64_t)cum[lo];
    code -= start * r;
    range = ((uint64_t)cum[lo + 1] == total) ? range - start * r : (uint64_t)(cum[lo + 1] - cum[lo]) * r;
    while (range < kTop) {
      range <<= 8;
      code = ((code << 8) | (uint64_t)s.get()) & (kFull - 1);
    }
    return lo;
  }
};

struct FileSink {
  FILE* f = nullptr;
  bool put(int b) { return fputc(b, f) != EOF; }
};
struct FileSource {
  FILE* f = nullptr;
  int get() {
    const int c = fgetc(f);
    return c == EOF ? 0 : c;
  }
};
struct MemSink {  // the caller guarantees room (tic_rcseg_bound)
  uint8_t* p = nullptr;
  bool put(int b) {
    *p++ = (uint8_t)b;
    return true;
  }
};
struct MemSource {  // bytes past the end read as zero
  const uint8_t *p = nullptr, *end = nullptr;
  int get() { return p < end ? *p++ : 0; }
};

// --- segmented stream, version 1 (include/tic.h) ---
constexpr uint32_t kSegMaxL = 16384;
constexpr size_t kSegHeader = 20;
const uint8_t kSegMagic[4] = {'T', 'I', 'C', 'S'};

bool seg_L_ok(uint32_t L) { return L >= 4 && L <= kSegMaxL && L % 4 == 0; }
uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }
void wr32(uint8_t* p, uint32_t v) {
  for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

// check_table plus the byte-symbol contract: at most 256 symbols, every frequency > 0
int check_seg_table(const int64_t* cum, size_t ncum, int64_t* total) {
  int rc = check_table(cum, ncum, total);
  if (rc) return rc;
  if (ncum > 257) return rc_fail(TIC_EINVAL, "segmented streams code byte symbols: at most 257 table entries");
  for (size_t i = 1; i < ncum; ++i)
    if (cum[i] == cum[i - 1]) return rc_fail(TIC_EINVAL, "segmented streams need every frequency > 0");
  return TIC_OK;
}

// --- segmented stream, version 2: K tables, symbol k of the stream under table k mod K ---
constexpr size_t kCtxHeader = 28;
constexpr size_t kCtxMaxK = 65536, kCtxMaxEntries = 262144;

// K rows of one ncum, each a check_seg_table table; totals[k] receives row k's total
int check_ctx_tables(const int64_t* tables, size_t K, size_t ncum, std::vector<int64_t>* totals) {
  if (!tables) return rc_fail(TIC_EINVAL, "invalid frequency table (null)");
  if (K < 1 || K > kCtxMaxK)
    return rc_fail(TIC_EINVAL, "context count " + std::to_string(K) + " must be in [1, 65536]");
  if (ncum < 2) return rc_fail(TIC_EINVAL, "invalid frequency table (needs >= 2 entries)");
  if (ncum > 257) return rc_fail(TIC_EINVAL, "segmented streams code byte symbols: at most 257 table entries");
  if (K * ncum > kCtxMaxEntries)
    return rc_fail(TIC_EINVAL, "context tables of " + std::to_string(K * ncum) + " entries exceed the limit of 262144");
  totals->resize(K);
  for (size_t k = 0; k < K; ++k) {
    const int rc = check_seg_table(tables + k * ncum, ncum, &(*totals)[k]);
    if (rc) {
      g_rc_err = "context " + std::to_string(k) + ": " + g_rc_err;
      return rc;
    }
  }
  return TIC_OK;
}

// CRC-32C of the K * ncum int64 entries, little-endian, row-major
uint32_t ctx_tables_crc(const int64_t* tables, size_t entries) {
  uint32_t crc = 0;
  uint8_t b[8 * 64];
  for (size_t at = 0; at < entries; at += 64) {
    const size_t m = std::min<size_t>(64, entries - at);
    for (size_t i = 0; i < m; ++i)
      for (int q = 0; q < 8; ++q) b[8 * i + q] = (uint8_t)((uint64_t)tables[at + i] >> (8 * q));
    crc = tic_crc32c(b, 8 * m, crc);
  }
  return crc;
}

// The framing both versions share around their headers: L, n, the length table behind a header
// of `header` bytes (nbytes >= header), the payload bytes.
int parse_framing(const uint8_t* buf, size_t nbytes, size_t header, uint32_t* L_out, uint64_t* n_out) {
  const uint32_t L = rd32(buf + 8);
  const uint64_t n = rd64(buf + 12);
  if (!seg_L_ok(L)) return rc_fail(TIC_EINVAL, "segmented stream: segment length " + std::to_string(L) + " must be a multiple of 4 in [4, 16384]");
  if (n == 0) return rc_fail(TIC_EINVAL, "segmented stream: no symbols");
  const uint64_t rest = nbytes - header;
  if (n > (UINT64_MAX >> 3) || (n + L - 1) / L > rest / 2)
    return rc_fail(TIC_EINVAL, "segmented stream: truncated inside the length table");
  const uint64_t S = (n + L - 1) / L;
  const uint8_t* lens = buf + header;
  uint64_t sum = 0;
  for (uint64_t j = 0; j < S; ++j) {
    const uint64_t len = (uint64_t)lens[2 * j] | (uint64_t)lens[2 * j + 1] << 8;
    const uint64_t cnt = j + 1 < S ? L : n - j * L;
    if (len > 3 * cnt + 4)
      return rc_fail(TIC_EINVAL, "segmented stream: segment " + std::to_string(j) + " claims " + std::to_string(len) +
                                     " bytes for " + std::to_string(cnt) + " symbols");
    sum += len;
  }
  if (sum != rest - 2 * S)
    return rc_fail(TIC_EINVAL, "segmented stream: segment lengths sum to " + std::to_string(sum) + " bytes, " +
                                   std::to_string(rest - 2 * S) + " follow the length table");
  if (L_out) *L_out = L;
  if (n_out) *n_out = n;
  return TIC_OK;
}

// --- segmented stream, version 3: K0 periodic contexts x the classes of the causal neighbours ---
constexpr size_t kNbrHeader = 36;

struct NbrModel {
  size_t K0 = 0, M = 0, ncum = 0;
  uint32_t eh = 0, ew = 0, C = 0, neighbours = 0;
};

int check_nbr_geometry(size_t K0, uint32_t eh, uint32_t ew, uint32_t C, uint32_t neighbours, const char* what) {
  if (neighbours != 1 && neighbours != 2)
    return rc_fail(TIC_EINVAL, std::string(what) + ": neighbours " + std::to_string(neighbours) + " must be 1 (W) or 2 (W and N)");
  if (eh < 1 || ew < 1 || C < 1 || eh > 65535 || ew > 65535 || C > 65535)
    return rc_fail(TIC_EINVAL, std::string(what) + ": code geometry " + std::to_string(eh) + " x " + std::to_string(ew) + " x " +
                                   std::to_string(C) + " must be in [1, 65535] each");
  const size_t M = neighbours == 1 ? 3 : 9;
  if (K0 < 1 || K0 > kCtxMaxEntries / (2 * M))
    return rc_fail(TIC_EINVAL, std::string(what) + ": context count " + std::to_string(K0) + " must be in [1, " +
                                   std::to_string(kCtxMaxEntries / (2 * M)) + "]");
  return TIC_OK;
}

// K0 * M rows of one ncum, each a check_seg_table table (rows the geometry never reaches included)
int check_nbr_tables(const int64_t* tables, const NbrModel& m, std::vector<int64_t>* totals) {
  if (!tables) return rc_fail(TIC_EINVAL, "invalid frequency table (null)");
  const int rc0 = check_nbr_geometry(m.K0, m.eh, m.ew, m.C, m.neighbours, "neighbour tables");
  if (rc0) return rc0;
  if (m.ncum < 2) return rc_fail(TIC_EINVAL, "invalid frequency table (needs >= 2 entries)");
  if (m.ncum > 257) return rc_fail(TIC_EINVAL, "segmented streams code byte symbols: at most 257 table entries");
  const size_t K = m.K0 * m.M;
  if (K * m.ncum > kCtxMaxEntries)
    return rc_fail(TIC_EINVAL, "neighbour tables of " + std::to_string(K * m.ncum) + " entries exceed the limit of 262144");
  totals->resize(K);
  for (size_t k = 0; k < K; ++k) {
    const int rc = check_seg_table(tables + k * m.ncum, m.ncum, &(*totals)[k]);
    if (rc) {
      g_rc_err = "context " + std::to_string(k / m.M) + ", neighbours " + std::to_string(k % m.M) + ": " + g_rc_err;
      return rc;
    }
  }
  return TIC_OK;
}

// The row of every symbol of one segment, in order: (c, w, h) and the K0 phase are counters that
// wrap, as on the device.  sym: the segment's own symbols, those before the current one valid (a
// neighbour in an earlier segment never counts, so nothing in front of the segment is read).
struct NbrWalk {
  const NbrModel& m;
  const uint8_t* sym;  // the segment's symbols: sym[0] is symbol b of the stream
  size_t b;            // the segment's first symbol
  size_t nsym, rowC;
  uint32_t c, w, h;
  size_t k0;
  NbrWalk(const NbrModel& m_, const uint8_t* sym_, size_t b_) : m(m_), sym(sym_), b(b_) {
    nsym = m.ncum - 1;
    rowC = (size_t)m.ew * m.C;
    const uint64_t p = (uint64_t)b % ((uint64_t)m.eh * rowC);
    c = (uint32_t)(p % m.C);
    w = (uint32_t)((p / m.C) % m.ew);
    h = (uint32_t)(p / rowC);
    k0 = b % m.K0;
  }
  size_t t(size_t j) const { return 1 + (2 * (size_t)sym[j - b] >= nsym ? 1 : 0); }
  size_t row(size_t i) const {  // of symbol i; then advance() before the next
    size_t nb = (m.neighbours >= 1 && w >= 1 && i - b >= m.C) ? t(i - m.C) : 0;
    if (m.neighbours == 2 && h >= 1 && i - b >= rowC) nb += 3 * t(i - rowC);
    return k0 * m.M + nb;
  }
  void advance() {
    if (++k0 == m.K0) k0 = 0;
    if (++c == m.C) {
      c = 0;
      if (++w == m.ew) {
        w = 0;
        if (++h == m.eh) h = 0;
      }
    }
  }
};

// --- symbol ranges (tic_rcseg_decode_range*) ---
int check_range(size_t n, size_t first, size_t count) {
  if (count == 0) return rc_fail(TIC_EINVAL, "symbol range: no symbols");
  if (first >= n || count > n - first)
    return rc_fail(TIC_EINVAL, "symbol range [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(count) +
                                   ") is not inside the stream's " + std::to_string(n) + " symbols");
  return TIC_OK;
}

// The segments j0 .. j1 that hold symbols [first, first + count) of a parsed container, one after
// another: [b, e) the segment's symbols, p / len its payload.  A segment is decoded from its
// start (the chain cannot begin in the middle): begin() is where its symbols go, straight into
// the output when the whole segment lies in the range, else a buffer of its own, from which
// commit() copies the part inside the range.  Payloads in front of j0 are skipped by their
// lengths, those behind j1 never looked at.
struct RangeWalk {
  const uint8_t *lens, *p;
  size_t n, L, first, count, j, j1, b = 0, e = 0, len = 0;
  uint8_t* out;
  std::vector<uint8_t> tmp;
  RangeWalk(const uint8_t* buf, size_t header, size_t n_, size_t L_, size_t first_, size_t count_, uint8_t* out_)
      : lens(buf + header), n(n_), L(L_), first(first_), count(count_), out(out_) {
    const size_t S = (n + L - 1) / L;
    p = lens + 2 * S;
    j1 = (first + count - 1) / L;
    for (j = 0; j < first / L; ++j) p += seg_len(j);
    load();
  }
  size_t seg_len(size_t k) const { return (size_t)lens[2 * k] | (size_t)lens[2 * k + 1] << 8; }
  void load() {
    if (j > j1) return;
    len = seg_len(j);
    b = j * L;
    e = std::min(std::min(n, b + L), first + count);  // nothing behind the range is decoded
  }
  bool more() const { return j <= j1; }
  void next() {
    p += len;
    ++j;
    load();
  }
  bool direct() const { return b >= first; }
  uint8_t* begin() {
    if (direct()) return out + (b - first);
    tmp.resize(e - b);
    return tmp.data();
  }
  void commit() {
    if (!direct()) memcpy(out, tmp.data() + (first - b), e - first);
  }
};
}  // namespace

struct tic_rc_encoder {
  EncCore<FileSink> c;
  bool closed = false;
};

struct tic_rc_decoder {
  DecCore<FileSource> c;
  bool closed = false;
};

extern "C" {

const char* tic_rc_last_error(void) { return g_rc_err.c_str(); }

int tic_rc_encoder_open(const char* path, tic_rc_encoder** out) {
  if (!path || !out) return rc_fail(TIC_EINVAL, "null argument");
  FILE* f = fopen(path, "wb");
  if (!f) return rc_fail(TIC_EIO, std::string("cannot open ") + path + ": " + strerror(errno));
  *out = new tic_rc_encoder();
  (*out)->c.s.f = f;
  return TIC_OK;
}

int tic_rc_encode(tic_rc_encoder* e, const int64_t* data, size_t n, const int64_t* cum, size_t ncum) {
  if (!e) return rc_fail(TIC_EINVAL, "null encoder");
  if (e->closed) return rc_fail(TIC_ESTATE, "encoder is closed");
  int64_t total = 0;
  int rc = check_table(cum, ncum, &total);
  if (rc) return rc;
  const int64_t nsym = (int64_t)ncum - 1;
  for (size_t i = 0; i < n; ++i) {
    const int64_t s = data[i];
    if (s < 0 || s >= nsym) return rc_fail(TIC_EINVAL, "symbol " + std::to_string(s) + " outside the table (cumFreq too short)");
    const uint64_t start = (uint64_t)cum[s], freq = (uint64_t)(cum[s + 1] - cum[s]);
    if (freq == 0) return rc_fail(TIC_EINVAL, "symbols with zero probability cannot be encoded");
    if (!e->c.symbol(start, freq, (uint64_t)total, cum[s + 1] == total)) return rc_fail(TIC_EIO, "write failed");
  }
  return TIC_OK;
}

int tic_rc_encoder_close(tic_rc_encoder* e) {
  if (!e) return rc_fail(TIC_EINVAL, "null encoder");
  if (e->closed) return TIC_OK;
  e->closed = true;
  bool ok = e->c.finish();
  if (fclose(e->c.s.f) != 0) ok = false;
  e->c.s.f = nullptr;
  return ok ? TIC_OK : rc_fail(TIC_EIO, "write failed");
}

void tic_rc_encoder_free(tic_rc_encoder* e) {
  if (!e) return;
  if (e->c.s.f) fclose(e->c.s.f);
  delete e;
}

int tic_rc_decoder_open(const char* path, tic_rc_decoder** out) {
  if (!path || !out) return rc_fail(TIC_EINVAL, "null argument");
  FILE* f = fopen(path, "rb");
  if (!f) return rc_fail(TIC_EIO, std::string("cannot open ") + path + ": " + strerror(errno));
  tic_rc_decoder* d = new tic_rc_decoder();
  d->c.s.f = f;
  d->c.start();
  *out = d;
  return TIC_OK;
}

int tic_rc_decode(tic_rc_decoder* d, size_t n, const int64_t* cum, size_t ncum, int64_t* out) {
  if (!d) return rc_fail(TIC_EINVAL, "null decoder");
  if (d->closed) return rc_fail(TIC_ESTATE, "decoder is closed");
  int64_t total = 0;
  int rc = check_table(cum, ncum, &total);
  if (rc) return rc;
  const int64_t nsym = (int64_t)ncum - 1;
  for (size_t i = 0; i < n; ++i) out[i] = d->c.symbol(cum, nsym, (uint64_t)total);
  return TIC_OK;
}

int tic_rc_decoder_close(tic_rc_decoder* d) {
  if (!d) return rc_fail(TIC_EINVAL, "null decoder");
  if (!d->closed && d->c.s.f) fclose(d->c.s.f);
  d->c.s.f = nullptr;
  d->closed = true;
  return TIC_OK;
}

void tic_rc_decoder_free(tic_rc_decoder* d) {
  if (!d) return;
  if (d->c.s.f) fclose(d->c.s.f);
  delete d;
}

// --- segmented stream ---

int tic_rcseg_bound(size_t n, uint32_t L, size_t* bytes) {
  if (!bytes) return rc_fail(TIC_EINVAL, "null argument");
  *bytes = 0;
  if (!seg_L_ok(L)) return rc_fail(TIC_EINVAL, "segment length " + std::to_string(L) + " must be a multiple of 4 in [4, 16384]");
  if (n == 0) return rc_fail(TIC_EINVAL, "a segmented stream holds at least one symbol");
  if (n > (SIZE_MAX >> 3)) return rc_fail(TIC_EINVAL, "too many symbols");
  const size_t S = (n + L - 1) / L;
  *bytes = kSegHeader + 2 * S + 3 * n + 4 * S;
  return TIC_OK;
}

int tic_rcseg_encode(const uint8_t* sym, size_t n, uint32_t L, const int64_t* cum, size_t ncum, uint8_t* out,
                     size_t cap, size_t* written) {
  if (!sym || !out || !written) return rc_fail(TIC_EINVAL, "null argument");
  *written = 0;
  size_t bound = 0;
  int rc = tic_rcseg_bound(n, L, &bound);
  if (rc) return rc;
  int64_t total = 0;
  if ((rc = check_seg_table(cum, ncum, &total))) return rc;
  if (cap < bound)
    return rc_fail(TIC_EINVAL, "output of " + std::to_string(cap) + " bytes is below tic_rcseg_bound (" + std::to_string(bound) + ")");
  const size_t S = (n + L - 1) / L, nsym = ncum - 1;
  memcpy(out, kSegMagic, 4);
  wr32(out + 4, 1);  // version 1, three zero bytes
  wr32(out + 8, L);
  wr32(out + 12, (uint32_t)((uint64_t)n & 0xFFFFFFFFu));
  wr32(out + 16, (uint32_t)((uint64_t)n >> 32));
  uint8_t* lens = out + kSegHeader;
  uint8_t* p = lens + 2 * S;
  for (size_t j = 0; j < S; ++j) {
    const size_t b = j * L, e = std::min(n, b + L);
    EncCore<MemSink> c;
    c.s.p = p;
    for (size_t i = b; i < e; ++i) {
      const size_t s = sym[i];
      if (s >= nsym) return rc_fail(TIC_EINVAL, "symbol " + std::to_string(s) + " outside the table (cumFreq too short)");
      c.symbol((uint64_t)cum[s], (uint64_t)(cum[s + 1] - cum[s]), (uint64_t)total, cum[s + 1] == total);
    }
    c.finish();
    const size_t len = (size_t)(c.s.p - p);
    lens[2 * j] = (uint8_t)(len & 0xFF);
    lens[2 * j + 1] = (uint8_t)(len >> 8);
    p = c.s.p;
  }
  *written = (size_t)(p - out);
  return TIC_OK;
}

int tic_rcseg_parse(const uint8_t* buf, size_t nbytes, uint32_t* L_out, uint64_t* n_out) {
  if (!buf) return rc_fail(TIC_EINVAL, "null argument");
  if (nbytes < kSegHeader) return rc_fail(TIC_EINVAL, "not a segmented stream: shorter than its 20-byte header");
  if (memcmp(buf, kSegMagic, 4) != 0) return rc_fail(TIC_EINVAL, "not a segmented stream: magic is not \"TICS\"");
  if (buf[4] != 1) return rc_fail(TIC_EINVAL, "segmented stream version " + std::to_string(buf[4]) + " is not supported");
  if (buf[5] || buf[6] || buf[7]) return rc_fail(TIC_EINVAL, "segmented stream: reserved bytes are not zero");
  return parse_framing(buf, nbytes, kSegHeader, L_out, n_out);
}

int tic_rcseg_decode_range(const uint8_t* buf, size_t nbytes, const int64_t* cum, size_t ncum, uint8_t* sym_out,
                           size_t n, size_t first, size_t count) {
  if (!sym_out) return rc_fail(TIC_EINVAL, "null argument");
  uint32_t L = 0;
  uint64_t hn = 0;
  int rc = tic_rcseg_parse(buf, nbytes, &L, &hn);
  if (rc) return rc;
  if (hn != (uint64_t)n)
    return rc_fail(TIC_EINVAL, "segmented stream holds " + std::to_string(hn) + " symbols, " + std::to_string(n) + " expected");
  int64_t total = 0;
  if ((rc = check_seg_table(cum, ncum, &total))) return rc;
  if ((rc = check_range(n, first, count))) return rc;
  RangeWalk rw(buf, kSegHeader, n, L, first, count, sym_out);
  for (; rw.more(); rw.next()) {
    DecCore<MemSource> c;
    c.s.p = rw.p;
    c.s.end = rw.p + rw.len;
    c.start();
    uint8_t* seg = rw.begin();
    for (size_t i = 0; i < rw.e - rw.b; ++i) seg[i] = (uint8_t)c.symbol(cum, (int64_t)ncum - 1, (uint64_t)total);
    rw.commit();
  }
  return TIC_OK;
}

int tic_rcseg_decode(const uint8_t* buf, size_t nbytes, const int64_t* cum, size_t ncum, uint8_t* sym_out, size_t n) {
  // n == 0 never passes: no container holds no symbols, so the count check fails first
  return tic_rcseg_decode_range(buf, nbytes, cum, ncum, sym_out, n, 0, n);
}

// --- segmented stream, version 2 ---

int tic_rcseg_bound_ctx(size_t n, uint32_t L, size_t* bytes) {
  const int rc = tic_rcseg_bound(n, L, bytes);
  if (rc) return rc;
  *bytes += kCtxHeader - kSegHeader;
  return TIC_OK;
}

int tic_rcseg_encode_ctx(const uint8_t* sym, size_t n, uint32_t L, const int64_t* tables, size_t K, size_t ncum,
                         uint8_t* out, size_t cap, size_t* written) {
  if (!sym || !out || !written) return rc_fail(TIC_EINVAL, "null argument");
  *written = 0;
  size_t bound = 0;
  int rc = tic_rcseg_bound_ctx(n, L, &bound);
  if (rc) return rc;
  std::vector<int64_t> totals;
  if ((rc = check_ctx_tables(tables, K, ncum, &totals))) return rc;
  if (cap < bound)
    return rc_fail(TIC_EINVAL, "output of " + std::to_string(cap) + " bytes is below tic_rcseg_bound_ctx (" + std::to_string(bound) + ")");
  const size_t S = (n + L - 1) / L, nsym = ncum - 1;
  memcpy(out, kSegMagic, 4);
  wr32(out + 4, 2);  // version 2, three zero bytes
  wr32(out + 8, L);
  wr32(out + 12, (uint32_t)((uint64_t)n & 0xFFFFFFFFu));
  wr32(out + 16, (uint32_t)((uint64_t)n >> 32));
  wr32(out + 20, (uint32_t)K);
  wr32(out + 24, ctx_tables_crc(tables, K * ncum));
  uint8_t* lens = out + kCtxHeader;
  uint8_t* p = lens + 2 * S;
  for (size_t j = 0; j < S; ++j) {
    const size_t b = j * L, e = std::min(n, b + L);
    EncCore<MemSink> c;
    c.s.p = p;
    size_t k = b % K;  // the context is a counter that wraps, as on the device
    for (size_t i = b; i < e; ++i) {
      const size_t s = sym[i];
      if (s >= nsym) return rc_fail(TIC_EINVAL, "symbol " + std::to_string(s) + " outside the table (cumFreq too short)");
      const int64_t* cum = tables + k * ncum;
      c.symbol((uint64_t)cum[s], (uint64_t)(cum[s + 1] - cum[s]), (uint64_t)totals[k], cum[s + 1] == totals[k]);
      if (++k == K) k = 0;
    }
    c.finish();
    const size_t len = (size_t)(c.s.p - p);
    lens[2 * j] = (uint8_t)(len & 0xFF);
    lens[2 * j + 1] = (uint8_t)(len >> 8);
    p = c.s.p;
  }
  *written = (size_t)(p - out);
  return TIC_OK;
}

int tic_rcseg_parse_ctx(const uint8_t* buf, size_t nbytes, uint32_t* L_out, uint64_t* n_out, uint32_t* K_out,
                        uint32_t* crc_out) {
  if (!buf) return rc_fail(TIC_EINVAL, "null argument");
  if (nbytes < kSegHeader) return rc_fail(TIC_EINVAL, "not a segmented stream: shorter than its 20-byte header");
  if (memcmp(buf, kSegMagic, 4) != 0) return rc_fail(TIC_EINVAL, "not a segmented stream: magic is not \"TICS\"");
  if (buf[4] != 2)
    return rc_fail(TIC_EINVAL, "segmented stream version " + std::to_string(buf[4]) + " is not a context stream (version 2)");
  if (buf[5] || buf[6] || buf[7]) return rc_fail(TIC_EINVAL, "segmented stream: reserved bytes are not zero");
  if (nbytes < kCtxHeader) return rc_fail(TIC_EINVAL, "context stream: shorter than its 28-byte header");
  const uint32_t K = rd32(buf + 20);
  if (K < 1 || K > kCtxMaxK)
    return rc_fail(TIC_EINVAL, "context stream: context count " + std::to_string(K) + " must be in [1, 65536]");
  const int rc = parse_framing(buf, nbytes, kCtxHeader, L_out, n_out);
  if (rc) return rc;
  if (K_out) *K_out = K;
  if (crc_out) *crc_out = rd32(buf + 24);
  return TIC_OK;
}

int tic_rcseg_decode_range_ctx(const uint8_t* buf, size_t nbytes, const int64_t* tables, size_t K, size_t ncum,
                               uint8_t* sym_out, size_t n, size_t first, size_t count) {
  if (!sym_out) return rc_fail(TIC_EINVAL, "null argument");
  uint32_t L = 0, hK = 0, hcrc = 0;
  uint64_t hn = 0;
  int rc = tic_rcseg_parse_ctx(buf, nbytes, &L, &hn, &hK, &hcrc);
  if (rc) return rc;
  if (hn != (uint64_t)n)
    return rc_fail(TIC_EINVAL, "segmented stream holds " + std::to_string(hn) + " symbols, " + std::to_string(n) + " expected");
  std::vector<int64_t> totals;
  if ((rc = check_ctx_tables(tables, K, ncum, &totals))) return rc;
  if ((size_t)hK != K)
    return rc_fail(TIC_EINVAL, "context stream was coded under " + std::to_string(hK) + " tables, " + std::to_string(K) + " given");
  if (hcrc != ctx_tables_crc(tables, K * ncum))
    return rc_fail(TIC_EINVAL, "context stream: the tables' CRC-32C differs from the header's (coded under other tables)");
  if ((rc = check_range(n, first, count))) return rc;
  RangeWalk rw(buf, kCtxHeader, n, L, first, count, sym_out);
  for (; rw.more(); rw.next()) {
    DecCore<MemSource> c;
    c.s.p = rw.p;
    c.s.end = rw.p + rw.len;
    c.start();
    uint8_t* seg = rw.begin();
    size_t k = rw.b % K;
    for (size_t i = 0; i < rw.e - rw.b; ++i) {
      seg[i] = (uint8_t)c.symbol(tables + k * ncum, (int64_t)ncum - 1, (uint64_t)totals[k]);
      if (++k == K) k = 0;
    }
    rw.commit();
  }
  return TIC_OK;
}

int tic_rcseg_decode_ctx(const uint8_t* buf, size_t nbytes, const int64_t* tables, size_t K, size_t ncum,
                         uint8_t* sym_out, size_t n) {
  return tic_rcseg_decode_range_ctx(buf, nbytes, tables, K, ncum, sym_out, n, 0, n);
}

// --- segmented stream, version 3 ---

int tic_rcseg_bound_nbr(size_t n, uint32_t L, size_t* bytes) {
  const int rc = tic_rcseg_bound(n, L, bytes);
  if (rc) return rc;
  *bytes += kNbrHeader - kSegHeader;
  return TIC_OK;
}

int tic_rcseg_encode_nbr(const uint8_t* sym, size_t n, uint32_t L, const int64_t* tables, size_t K0,
                         uint32_t neighbours, size_t ncum, uint32_t eh, uint32_t ew, uint32_t C, uint8_t* out,
                         size_t cap, size_t* written) {
  if (!sym || !out || !written) return rc_fail(TIC_EINVAL, "null argument");
  *written = 0;
  size_t bound = 0;
  int rc = tic_rcseg_bound_nbr(n, L, &bound);
  if (rc) return rc;
  NbrModel m;
  m.K0 = K0, m.M = neighbours == 1 ? 3 : 9, m.ncum = ncum, m.eh = eh, m.ew = ew, m.C = C, m.neighbours = neighbours;
  std::vector<int64_t> totals;
  if ((rc = check_nbr_tables(tables, m, &totals))) return rc;
  if (cap < bound)
    return rc_fail(TIC_EINVAL, "output of " + std::to_string(cap) + " bytes is below tic_rcseg_bound_nbr (" + std::to_string(bound) + ")");
  const size_t S = (n + L - 1) / L, nsym = ncum - 1;
  for (size_t i = 0; i < n; ++i)  // before any row is derived from a symbol
    if (sym[i] >= nsym) return rc_fail(TIC_EINVAL, "symbol " + std::to_string(sym[i]) + " outside the table (cumFreq too short)");
  memcpy(out, kSegMagic, 4);
  wr32(out + 4, 3);  // version 3, three zero bytes
  wr32(out + 8, L);
  wr32(out + 12, (uint32_t)((uint64_t)n & 0xFFFFFFFFu));
  wr32(out + 16, (uint32_t)((uint64_t)n >> 32));
  wr32(out + 20, (uint32_t)K0);
  wr32(out + 24, ctx_tables_crc(tables, K0 * m.M * ncum));
  wr32(out + 28, eh | ew << 16);
  wr32(out + 32, C | neighbours << 16);  // byte 35 stays zero
  uint8_t* lens = out + kNbrHeader;
  uint8_t* p = lens + 2 * S;
  for (size_t j = 0; j < S; ++j) {
    const size_t b = j * L, e = std::min(n, b + L);
    EncCore<MemSink> c;
    c.s.p = p;
    NbrWalk walk(m, sym + b, b);
    for (size_t i = b; i < e; ++i) {
      const size_t s = sym[i], k = walk.row(i);
      const int64_t* cum = tables + k * ncum;
      c.symbol((uint64_t)cum[s], (uint64_t)(cum[s + 1] - cum[s]), (uint64_t)totals[k], cum[s + 1] == totals[k]);
      walk.advance();
    }
    c.finish();
    const size_t len = (size_t)(c.s.p - p);
    lens[2 * j] = (uint8_t)(len & 0xFF);
    lens[2 * j + 1] = (uint8_t)(len >> 8);
    p = c.s.p;
  }
  *written = (size_t)(p - out);
  return TIC_OK;
}

int tic_rcseg_parse_nbr(const uint8_t* buf, size_t nbytes, uint32_t* L_out, uint64_t* n_out, uint32_t* K0_out,
                        uint32_t* crc_out, uint32_t* eh_out, uint32_t* ew_out, uint32_t* C_out,
                        uint32_t* neighbours_out) {
  if (!buf) return rc_fail(TIC_EINVAL, "null argument");
  if (nbytes < kSegHeader) return rc_fail(TIC_EINVAL, "not a segmented stream: shorter than its 20-byte header");
  if (memcmp(buf, kSegMagic, 4) != 0) return rc_fail(TIC_EINVAL, "not a segmented stream: magic is not \"TICS\"");
  if (buf[4] != 3)
    return rc_fail(TIC_EINVAL, "segmented stream version " + std::to_string(buf[4]) + " is not a neighbour stream (version 3)");
  if (buf[5] || buf[6] || buf[7]) return rc_fail(TIC_EINVAL, "segmented stream: reserved bytes are not zero");
  if (nbytes < kNbrHeader) return rc_fail(TIC_EINVAL, "neighbour stream: shorter than its 36-byte header");
  if (buf[35]) return rc_fail(TIC_EINVAL, "neighbour stream: reserved byte is not zero");
  const uint32_t K0 = rd32(buf + 20);
  const uint32_t eh = buf[28] | (uint32_t)buf[29] << 8, ew = buf[30] | (uint32_t)buf[31] << 8,
                 C = buf[32] | (uint32_t)buf[33] << 8, nb = buf[34];
  int rc = check_nbr_geometry(K0, eh, ew, C, nb, "neighbour stream");
  if (rc) return rc;
  if ((rc = parse_framing(buf, nbytes, kNbrHeader, L_out, n_out))) return rc;
  if (K0_out) *K0_out = K0;
  if (crc_out) *crc_out = rd32(buf + 24);
  if (eh_out) *eh_out = eh;
  if (ew_out) *ew_out = ew;
  if (C_out) *C_out = C;
  if (neighbours_out) *neighbours_out = nb;
  return TIC_OK;
}

int tic_rcseg_decode_range_nbr(const uint8_t* buf, size_t nbytes, const int64_t* tables, size_t K0,
                               uint32_t neighbours, size_t ncum, uint32_t eh, uint32_t ew, uint32_t C,
                               uint8_t* sym_out, size_t n, size_t first, size_t count) {
  if (!sym_out) return rc_fail(TIC_EINVAL, "null argument");
  uint32_t L = 0, hK0 = 0, hcrc = 0, heh = 0, hew = 0, hC = 0, hnb = 0;
  uint64_t hn = 0;
  int rc = tic_rcseg_parse_nbr(buf, nbytes, &L, &hn, &hK0, &hcrc, &heh, &hew, &hC, &hnb);
  if (rc) return rc;
  if (hn != (uint64_t)n)
    return rc_fail(TIC_EINVAL, "segmented stream holds " + std::to_string(hn) + " symbols, " + std::to_string(n) + " expected");
  NbrModel m;
  m.K0 = K0, m.M = neighbours == 1 ? 3 : 9, m.ncum = ncum, m.eh = eh, m.ew = ew, m.C = C, m.neighbours = neighbours;
  std::vector<int64_t> totals;
  if ((rc = check_nbr_tables(tables, m, &totals))) return rc;
  if ((size_t)hK0 != K0)
    return rc_fail(TIC_EINVAL, "neighbour stream was coded under " + std::to_string(hK0) + " contexts, " + std::to_string(K0) + " given");
  if (heh != eh || hew != ew || hC != C)
    return rc_fail(TIC_EINVAL, "neighbour stream was coded for the geometry " + std::to_string(heh) + " x " + std::to_string(hew) +
                                   " x " + std::to_string(hC) + ", " + std::to_string(eh) + " x " + std::to_string(ew) + " x " +
                                   std::to_string(C) + " given");
  if (hnb != neighbours)
    return rc_fail(TIC_EINVAL, "neighbour stream was coded with neighbours " + std::to_string(hnb) + ", " + std::to_string(neighbours) + " given");
  if (hcrc != ctx_tables_crc(tables, K0 * m.M * ncum))
    return rc_fail(TIC_EINVAL, "neighbour stream: the tables' CRC-32C differs from the header's (coded under other tables)");
  if ((rc = check_range(n, first, count))) return rc;
  RangeWalk rw(buf, kNbrHeader, n, L, first, count, sym_out);
  for (; rw.more(); rw.next()) {
    DecCore<MemSource> c;
    c.s.p = rw.p;
    c.s.end = rw.p + rw.len;
    c.start();
    uint8_t* seg = rw.begin();
    NbrWalk walk(m, seg, rw.b);
    for (size_t i = rw.b; i < rw.e; ++i) {
      const size_t k = walk.row(i);
      seg[i - rw.b] = (uint8_t)c.symbol(tables + k * ncum, (int64_t)ncum - 1, (uint64_t)totals[k]);
      walk.advance();
    }
    rw.commit();
  }
  return TIC_OK;
}

int tic_rcseg_decode_nbr(const uint8_t* buf, size_t nbytes, const int64_t* tables, size_t K0, uint32_t neighbours,
                         size_t ncum, uint32_t eh, uint32_t ew, uint32_t C, uint8_t* sym_out, size_t n) {
  return tic_rcseg_decode_range_nbr(buf, nbytes, tables, K0, neighbours, ncum, eh, ew, C, sym_out, n, 0, n);
}

// The segments and payload bytes a symbol range needs, from the header and the length table alone.
int tic_rcseg_range_extent(const uint8_t* buf, size_t nbytes, size_t first, size_t count, size_t* j0_out, size_t* nj_out,
                           size_t* byte_off, size_t* byte_len) {
  if (!buf) return rc_fail(TIC_EINVAL, "null argument");
  if (nbytes < kSegHeader) return rc_fail(TIC_EINVAL, "not a segmented stream: shorter than its 20-byte header");
  if (memcmp(buf, kSegMagic, 4) != 0) return rc_fail(TIC_EINVAL, "not a segmented stream: magic is not \"TICS\"");
  const size_t header = buf[4] == 1 ? kSegHeader : buf[4] == 2 ? kCtxHeader : buf[4] == 3 ? kNbrHeader : 0;
  if (!header) return rc_fail(TIC_EINVAL, "segmented stream version " + std::to_string(buf[4]) + " is not supported");
  if (buf[5] || buf[6] || buf[7]) return rc_fail(TIC_EINVAL, "segmented stream: reserved bytes are not zero");
  if (nbytes < header)
    return rc_fail(TIC_EINVAL, "segmented stream: shorter than its " + std::to_string(header) + "-byte header");
  const uint32_t L = rd32(buf + 8);
  const uint64_t n = rd64(buf + 12);
  if (!seg_L_ok(L)) return rc_fail(TIC_EINVAL, "segmented stream: segment length " + std::to_string(L) + " must be a multiple of 4 in [4, 16384]");
  if (n == 0) return rc_fail(TIC_EINVAL, "segmented stream: no symbols");
  if (n > (UINT64_MAX >> 3) || (n + L - 1) / L > (nbytes - header) / 2)
    return rc_fail(TIC_EINVAL, "segmented stream: truncated inside the length table");
  const int rc = check_range((size_t)n, first, count);
  if (rc) return rc;
  const uint64_t S = (n + L - 1) / L, j0 = first / L, j1 = (first + count - 1) / L;
  const uint8_t* lens = buf + header;
  uint64_t off = header + 2 * S, len = 0;
  for (uint64_t j = 0; j <= j1; ++j) {
    const uint64_t l = (uint64_t)lens[2 * j] | (uint64_t)lens[2 * j + 1] << 8;
    if (j < j0) off += l;
    else len += l;
  }
  if (j0_out) *j0_out = (size_t)j0;
  if (nj_out) *nj_out = (size_t)(j1 - j0 + 1);
  if (byte_off) *byte_off = (size_t)off;
  if (byte_len) *byte_len = (size_t)len;
  return TIC_OK;
}

}  // extern "C"

// --- "TICA" version 1: version 3's context model under tables fitted to the stream itself and
// carried in the container (include/tic.h) ---
namespace {
const uint8_t kEmbMagic[4] = {'T', 'I', 'C', 'A'};
constexpr size_t kEmbHeader = 40;
constexpr uint32_t kEmbTotal = 4096;
constexpr uint64_t kEmbMaxCount = 1ull << 40;

struct EmbHead {
  NbrModel m;
  uint32_t L = 0;
  uint64_t n = 0;
  size_t T = 0, nsym = 0;
  size_t header() const { return kEmbHeader + T; }  // the length table starts here
};

// The model's limits; fills m (ncum = nsym + 1, M = 3^neighbours).
int emb_model(size_t K0, uint32_t neighbours, size_t nsym, uint32_t eh, uint32_t ew, uint32_t C, const char* what,
              NbrModel* m) {
  if (neighbours > 2)
    return rc_fail(TIC_EINVAL, std::string(what) + ": neighbours " + std::to_string(neighbours) + " must be 0, 1 (W) or 2 (W and N)");
  if (nsym < 2 || nsym > 256)
    return rc_fail(TIC_EINVAL, std::string(what) + ": symbol count " + std::to_string(nsym) + " must be in [2, 256]");
  if (eh < 1 || ew < 1 || C < 1 || eh > 65535 || ew > 65535 || C > 65535)
    return rc_fail(TIC_EINVAL, std::string(what) + ": code geometry " + std::to_string(eh) + " x " + std::to_string(ew) + " x " +
                                   std::to_string(C) + " must be in [1, 65535] each");
  const size_t M = neighbours == 0 ? 1 : neighbours == 1 ? 3 : 9;
  if (K0 < 1 || K0 > kCtxMaxEntries / (M * (nsym + 1)))
    return rc_fail(TIC_EINVAL, std::string(what) + ": context count " + std::to_string(K0) + " must be in [1, " +
                                   std::to_string(kCtxMaxEntries / (M * (nsym + 1))) + "]");
  m->K0 = K0, m->M = M, m->ncum = nsym + 1, m->eh = eh, m->ew = ew, m->C = C, m->neighbours = neighbours;
  return TIC_OK;
}

// Header and table block of a container (buf[0 .. 40 + T) must be present, nothing behind it is
// read); tables, when not NULL, receives the K0*M cumulative rows.
int emb_head(const uint8_t* buf, size_t nbytes, EmbHead* hd, int64_t* tables) {
  if (!buf) return rc_fail(TIC_EINVAL, "null argument");
  if (nbytes < 4 || memcmp(buf, kEmbMagic, 4) != 0)
    return rc_fail(TIC_EINVAL, "not an embedded-table stream: magic is not \"TICA\"");
  if (nbytes < kEmbHeader) return rc_fail(TIC_EINVAL, "embedded-table stream: shorter than its 40-byte header");
  if (buf[4] != 1) return rc_fail(TIC_EINVAL, "embedded-table stream version " + std::to_string(buf[4]) + " is not supported");
  if (buf[30] || buf[31]) return rc_fail(TIC_EINVAL, "embedded-table stream: reserved bytes are not zero");
  const uint32_t nsym = buf[6] | (uint32_t)buf[7] << 8, K0 = rd32(buf + 20);
  const uint32_t eh = buf[24] | (uint32_t)buf[25] << 8, ew = buf[26] | (uint32_t)buf[27] << 8,
                 C = buf[28] | (uint32_t)buf[29] << 8;
  int rc = emb_model(K0, buf[5], nsym, eh, ew, C, "embedded-table stream", &hd->m);
  if (rc) return rc;
  hd->L = rd32(buf + 8);
  hd->n = rd64(buf + 12);
  hd->nsym = nsym;
  if (!seg_L_ok(hd->L))
    return rc_fail(TIC_EINVAL, "segmented stream: segment length " + std::to_string(hd->L) + " must be a multiple of 4 in [4, 16384]");
  if (hd->n == 0) return rc_fail(TIC_EINVAL, "segmented stream: no symbols");
  const size_t K = hd->m.K0 * hd->m.M;
  hd->T = K * (nsym - 1) * 2;
  if (rd32(buf + 32) != hd->T)
    return rc_fail(TIC_EINVAL, "embedded-table stream: table block of " + std::to_string(rd32(buf + 32)) + " bytes, " +
                                   std::to_string(hd->T) + " expected for its model");
  if (nbytes - kEmbHeader < hd->T) return rc_fail(TIC_EINVAL, "embedded-table stream: truncated inside the table block");
  const uint8_t* tb = buf + kEmbHeader;
  if (rd32(buf + 36) != tic_crc32c(tb, hd->T, 0))
    return rc_fail(TIC_EINVAL, "embedded-table stream: the table block's CRC-32C differs from the header's");
  for (size_t r = 0; r < K; ++r) {
    uint32_t sum = 0;
    if (tables) tables[r * (nsym + 1)] = 0;
    for (size_t s = 0; s + 1 < nsym; ++s) {
      const uint8_t* p = tb + (r * (nsym - 1) + s) * 2;
      const uint32_t f = p[0] | (uint32_t)p[1] << 8;
      if (f == 0)
        return rc_fail(TIC_EINVAL, "embedded-table stream: row " + std::to_string(r) + " has a zero frequency");
      sum += f;
      if (sum >= kEmbTotal)
        return rc_fail(TIC_EINVAL, "embedded-table stream: row " + std::to_string(r) + " sums to more than 4095");
      if (tables) tables[r * (nsym + 1) + s + 1] = sum;
    }
    if (tables) tables[r * (nsym + 1) + nsym] = kEmbTotal;
  }
  return TIC_OK;
}

int emb_count(const uint8_t* sym, size_t n, uint32_t L, const NbrModel& m, uint64_t* counts) {
  const size_t nsym = m.ncum - 1;
  memset(counts, 0, m.K0 * m.M * nsym * sizeof(uint64_t));
  for (size_t i = 0; i < n; ++i)  // before any row is derived from a symbol
    if (sym[i] >= nsym) return rc_fail(TIC_EINVAL, "symbol " + std::to_string(sym[i]) + " outside the table (cumFreq too short)");
  for (size_t b = 0; b < n; b += L) {
    const size_t e = std::min(n, b + L);
    NbrWalk walk(m, sym + b, b);
    for (size_t i = b; i < e; ++i) {
      ++counts[walk.row(i) * nsym + sym[i]];
      walk.advance();
    }
  }
  return TIC_OK;
}

// One row of the fit rule (include/tic.h): frequencies f[0 .. nsym) summing to 4096, each >= 1.
int emb_fit_row(const uint64_t* c, size_t nsym, uint32_t* f) {
  uint64_t nr = 0;
  for (size_t s = 0; s < nsym; ++s) {
    if (c[s] > kEmbMaxCount) return rc_fail(TIC_EINVAL, "a count above 2^40");
    nr += c[s];
  }
  if (nr == 0) {
    for (size_t s = 0; s < nsym; ++s) f[s] = (uint32_t)(kEmbTotal * (s + 1) / nsym - kEmbTotal * s / nsym);
    return TIC_OK;
  }
  uint32_t sum = 0;
  size_t best = 0;
  for (size_t s = 0; s < nsym; ++s) {
    f[s] = 1 + (uint32_t)(c[s] * (uint64_t)(kEmbTotal - nsym) / nr);
    sum += f[s];
    if (c[s] > c[best]) best = s;
  }
  f[best] += kEmbTotal - sum;
  return TIC_OK;
}
}  // namespace

extern "C" {

int tic_rcseg_count_nbr(const uint8_t* sym, size_t n, uint32_t L, size_t K0, uint32_t neighbours, size_t nsym,
                        uint32_t eh, uint32_t ew, uint32_t C, uint64_t* counts) {
  if (!sym || !counts) return rc_fail(TIC_EINVAL, "null argument");
  if (!seg_L_ok(L)) return rc_fail(TIC_EINVAL, "segment length " + std::to_string(L) + " must be a multiple of 4 in [4, 16384]");
  NbrModel m;
  const int rc = emb_model(K0, neighbours, nsym, eh, ew, C, "context model", &m);
  if (rc) return rc;
  return emb_count(sym, n, L, m, counts);
}

int tic_rcseg_fit_tables(const uint64_t* counts, size_t K, size_t nsym, int64_t* tables) {
  if (!counts || !tables) return rc_fail(TIC_EINVAL, "null argument");
  if (nsym < 2 || nsym > 256) return rc_fail(TIC_EINVAL, "symbol count " + std::to_string(nsym) + " must be in [2, 256]");
  if (K < 1 || K > kCtxMaxEntries / (nsym + 1))
    return rc_fail(TIC_EINVAL, "row count " + std::to_string(K) + " must be in [1, " + std::to_string(kCtxMaxEntries / (nsym + 1)) + "]");
  uint32_t f[256];
  for (size_t r = 0; r < K; ++r) {
    const int rc = emb_fit_row(counts + r * nsym, nsym, f);
    if (rc) return rc;
    int64_t* row = tables + r * (nsym + 1);
    row[0] = 0;
    for (size_t s = 0; s < nsym; ++s) row[s + 1] = row[s] + f[s];
  }
  return TIC_OK;
}

int tic_rcseg_bound_emb(size_t n, uint32_t L, size_t K0, uint32_t neighbours, size_t nsym, size_t* bytes) {
  int rc = tic_rcseg_bound(n, L, bytes);
  if (rc) return rc;
  NbrModel m;
  if ((rc = emb_model(K0, neighbours, nsym, 1, 1, 1, "context model", &m))) {
    *bytes = 0;
    return rc;
  }
  *bytes += kEmbHeader - kSegHeader + m.K0 * m.M * (nsym - 1) * 2;
  return TIC_OK;
}

int tic_rcseg_encode_emb(const uint8_t* sym, size_t n, uint32_t L, size_t K0, uint32_t neighbours, size_t nsym,
                         uint32_t eh, uint32_t ew, uint32_t C, uint8_t* out, size_t cap, size_t* written) {
  if (!sym || !out || !written) return rc_fail(TIC_EINVAL, "null argument");
  *written = 0;
  size_t bound = 0;
  int rc = tic_rcseg_bound_emb(n, L, K0, neighbours, nsym, &bound);
  if (rc) return rc;
  NbrModel m;
  if ((rc = emb_model(K0, neighbours, nsym, eh, ew, C, "context model", &m))) return rc;
  if (cap < bound)
    return rc_fail(TIC_EINVAL, "output of " + std::to_string(cap) + " bytes is below tic_rcseg_bound_emb (" + std::to_string(bound) + ")");
  const size_t K = m.K0 * m.M, ncum = m.ncum, T = K * (nsym - 1) * 2, S = (n + L - 1) / L;
  std::vector<uint64_t> counts(K * nsym);
  if ((rc = emb_count(sym, n, L, m, counts.data()))) return rc;
  std::vector<int64_t> tables(K * ncum);
  if ((rc = tic_rcseg_fit_tables(counts.data(), K, nsym, tables.data()))) return rc;
  memcpy(out, kEmbMagic, 4);
  out[4] = 1;
  out[5] = (uint8_t)neighbours;
  out[6] = (uint8_t)(nsym & 0xFF), out[7] = (uint8_t)(nsym >> 8);
  wr32(out + 8, L);
  wr32(out + 12, (uint32_t)((uint64_t)n & 0xFFFFFFFFu));
  wr32(out + 16, (uint32_t)((uint64_t)n >> 32));
  wr32(out + 20, (uint32_t)K0);
  wr32(out + 24, eh | ew << 16);
  wr32(out + 28, C);  // bytes 30, 31 stay zero
  wr32(out + 32, (uint32_t)T);
  uint8_t* tb = out + kEmbHeader;
  for (size_t r = 0; r < K; ++r)
    for (size_t s = 0; s + 1 < nsym; ++s) {
      const uint32_t f = (uint32_t)(tables[r * ncum + s + 1] - tables[r * ncum + s]);
      tb[(r * (nsym - 1) + s) * 2] = (uint8_t)(f & 0xFF);
      tb[(r * (nsym - 1) + s) * 2 + 1] = (uint8_t)(f >> 8);
    }
  wr32(out + 36, tic_crc32c(tb, T, 0));
  uint8_t* lens = tb + T;
  uint8_t* p = lens + 2 * S;
  for (size_t j = 0; j < S; ++j) {
    const size_t b = j * L, e = std::min(n, b + L);
    EncCore<MemSink> c;
    c.s.p = p;
    NbrWalk walk(m, sym + b, b);
    for (size_t i = b; i < e; ++i) {
      const size_t s = sym[i];
      const int64_t* cum = tables.data() + walk.row(i) * ncum;
      c.symbol((uint64_t)cum[s], (uint64_t)(cum[s + 1] - cum[s]), kEmbTotal, cum[s + 1] == kEmbTotal);
      walk.advance();
    }
    c.finish();
    const size_t len = (size_t)(c.s.p - p);
    lens[2 * j] = (uint8_t)(len & 0xFF);
    lens[2 * j + 1] = (uint8_t)(len >> 8);
    p = c.s.p;
  }
  *written = (size_t)(p - out);
  return TIC_OK;
}

int tic_rcseg_parse_emb(const uint8_t* buf, size_t nbytes, uint32_t* L_out, uint64_t* n_out, uint32_t* K0_out,
                        uint32_t* eh_out, uint32_t* ew_out, uint32_t* C_out, uint32_t* neighbours_out,
                        uint32_t* nsym_out, int64_t* tables) {
  EmbHead hd;
  int rc = emb_head(buf, nbytes, &hd, nullptr);
  if (rc) return rc;
  if ((rc = parse_framing(buf, nbytes, hd.header(), nullptr, nullptr))) return rc;
  if (tables) (void)emb_head(buf, nbytes, &hd, tables);  // outputs only once the whole container is valid
  if (L_out) *L_out = hd.L;
  if (n_out) *n_out = hd.n;
  if (K0_out) *K0_out = (uint32_t)hd.m.K0;
  if (eh_out) *eh_out = hd.m.eh;
  if (ew_out) *ew_out = hd.m.ew;
  if (C_out) *C_out = hd.m.C;
  if (neighbours_out) *neighbours_out = hd.m.neighbours;
  if (nsym_out) *nsym_out = (uint32_t)hd.nsym;
  return TIC_OK;
}

int tic_rcseg_decode_range_emb(const uint8_t* buf, size_t nbytes, uint8_t* sym_out, size_t n, size_t first,
                               size_t count) {
  if (!sym_out) return rc_fail(TIC_EINVAL, "null argument");
  EmbHead hd;
  int rc = emb_head(buf, nbytes, &hd, nullptr);
  if (rc) return rc;
  if ((rc = parse_framing(buf, nbytes, hd.header(), nullptr, nullptr))) return rc;
  if (hd.n != (uint64_t)n)
    return rc_fail(TIC_EINVAL, "segmented stream holds " + std::to_string(hd.n) + " symbols, " + std::to_string(n) + " expected");
  if ((rc = check_range(n, first, count))) return rc;
  const NbrModel& m = hd.m;
  std::vector<int64_t> tables(m.K0 * m.M * m.ncum);
  (void)emb_head(buf, nbytes, &hd, tables.data());
  RangeWalk rw(buf, hd.header(), n, hd.L, first, count, sym_out);
  for (; rw.more(); rw.next()) {
    DecCore<MemSource> c;
    c.s.p = rw.p;
    c.s.end = rw.p + rw.len;
    c.start();
    uint8_t* seg = rw.begin();
    NbrWalk walk(m, seg, rw.b);
    for (size_t i = rw.b; i < rw.e; ++i) {
      seg[i - rw.b] = (uint8_t)c.symbol(tables.data() + walk.row(i) * m.ncum, (int64_t)m.ncum - 1, kEmbTotal);
      walk.advance();
    }
    rw.commit();
  }
  return TIC_OK;
}

int tic_rcseg_decode_emb(const uint8_t* buf, size_t nbytes, uint8_t* sym_out, size_t n) {
  return tic_rcseg_decode_range_emb(buf, nbytes, sym_out, n, 0, n);
}

int tic_rcseg_range_extent_emb(const uint8_t* buf, size_t nbytes, size_t first, size_t count, size_t* j0_out,
                               size_t* nj_out, size_t* byte_off, size_t* byte_len) {
  EmbHead hd;
  int rc = emb_head(buf, nbytes, &hd, nullptr);
  if (rc) return rc;
  const size_t header = hd.header();
  const uint64_t n = hd.n, L = hd.L;
  if (n > (UINT64_MAX >> 3) || (n + L - 1) / L > (nbytes - header) / 2)
    return rc_fail(TIC_EINVAL, "segmented stream: truncated inside the length table");
  if ((rc = check_range((size_t)n, first, count))) return rc;
  const uint64_t S = (n + L - 1) / L, j0 = first / L, j1 = (first + count - 1) / L;
  const uint8_t* lens = buf + header;
  uint64_t off = header + 2 * S, len = 0;
  for (uint64_t j = 0; j <= j1; ++j) {
    const uint64_t l = (uint64_t)lens[2 * j] | (uint64_t)lens[2 * j + 1] << 8;
    if (j < j0) off += l;
    else len += l;
  }
  if (j0_out) *j0_out = (size_t)j0;
  if (nj_out) *nj_out = (size_t)(j1 - j0 + 1);
  if (byte_off) *byte_off = (size_t)off;
  if (byte_len) *byte_len = (size_t)len;
  return TIC_OK;
}

}  // extern "C"
