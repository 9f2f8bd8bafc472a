// tic_entropy.cpp — the segmented range-coder stream (include/tic.h, "TICS" version 1) coded on
// the device, and its C-ABI entries.
//
// The single-stream coder of range_coder.cpp is one latency chain per image.  A segmented stream
// cuts the symbols into segments of L that are independent range-coder streams, so the chain is
// L symbols long and there are n / L of them:
//
//   ent_encode_kernel       ONE SEGMENT PER LANE, 64-lane workgroups (a latency chain, not a
//                           bandwidth kernel: waves spread over the CUs).  The coder state (low,
//                           range, cache, pending) stays in registers; carries are resolved with
//                           the host's cache + pending-0xFF scheme, so no stored byte is revisited.
//                           A lane reads its own symbols with 16-byte loads once its address is
//                           aligned and writes its payload, four bytes per store, into its own
//                           slot of the scratch (stride 3L + 4, the worst case) and its length
//                           beside it.
//   ent_seg_scan_kernel     one workgroup per stream: exclusive scan of its segment lengths, the
//                           container size into d_sizes (UINT64_MAX when a lane met a symbol
//                           outside the table)
//   ent_stream_scan_kernel  one workgroup: exclusive scan over the streams
//   ent_gather_kernel       one workgroup per segment: consecutive threads copy consecutive
//                           payload bytes to their final place; the first segment's workgroup also
//                           writes the header, every workgroup its u16 length
//
// and the decoder: ent_dec_header_kernel (checks each header against the caller's count and
// size), ent_stream_scan_kernel over the segment counts, ent_dec_scan_kernel (segment offsets;
// zero-fills a stream it cannot decode) and ent_decode_kernel (one segment per lane, grid-stride).
//
// Arithmetic is the host's, exactly: range needs 33 bits (it starts at 2^32) and is held in 64;
// range / total is a shift when the total is a power of two and a true division otherwise; the
// decoder's code / r is a true 32-bit division (r = 2^32 only when the total is 1, where the
// quotient is 0).  The decoder finds the symbol of a value through a byte table in LDS built by
// each workgroup from the cumulative table (totals up to 65536), else by the host's binary search.
//
// The model (at most 257 cumulative counts) and the per-stream tables travel BY VALUE in kernel
// arguments, as in tic_image_batch.cpp: nothing is uploaded, host arrays are free on return and
// no call synchronises.  The per-stream records a later kernel needs are written to the caller's
// scratch by a kernel that received them by value.  tic_entropy_set_table therefore only keeps
// the validated table on the host, keyed by the handle; the handle struct belongs to
// tic_runtime.cpp, which stays as the shipped tuning states were stamped, so tic_destroy is
// wrapped below to drop that entry with the handle.
//
// This file closes the one translation unit of the host runtime (it includes tic_msssim.cpp).
#define tic_destroy tic_destroy_runtime_
#include "tic_msssim.cpp"
#undef tic_destroy

#include <mutex>

namespace tic {

constexpr int kEntStreams = 64;  // streams per by-value table
constexpr uint32_t kEntMaxL = 16384;
constexpr uint32_t kEntBad = 0xFFFFFFFFu;
constexpr uint32_t kEntLutMax = 65536;

struct EntModel {
  uint32_t cum[257];
  int nsym;
  int shift;  // log2(total) when the total is a power of two, else -1
};

struct EntChunk {
  long long in_off[kEntStreams], in_size[kEntStreams], count[kEntStreams], out_off[kEntStreams];
  long long seg_base[kEntStreams + 1];
  int n, first, last;  // last: this chunk ends the list (seg_base[n] is the total)
};

struct EntRec {
  long long in_off, in_size, count, out_off;
  uint32_t L, valid;
};

__host__ __device__ __forceinline__ uint32_t ent_stride(uint32_t L) { return 3 * L + 4; }

// Last i with base[i] <= v, base in device memory (ragged_find's contract).
__device__ __forceinline__ int ent_find(const unsigned long long* base, int n, unsigned long long v) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (base[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Inclusive scan of one value per thread over a 256-thread workgroup (s: 256 entries).
__device__ __forceinline__ unsigned long long ent_block_scan(unsigned long long v, unsigned long long* s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const unsigned long long o = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += o;
    __syncthreads();
  }
  const unsigned long long r = s[t];
  __syncthreads();
  return r;
}

// The by-value records of one chunk of streams into the scratch.
__global__ void __launch_bounds__(64) ent_put_kernel(const EntChunk t, uint32_t L, EntRec* __restrict__ rec,
                                                     unsigned long long* __restrict__ seg_base) {
  const int k = threadIdx.x;
  if (k < t.n) {
    EntRec r;
    r.in_off = t.in_off[k];
    r.in_size = t.in_size[k];
    r.count = t.count[k];
    r.out_off = t.out_off[k];
    r.L = L;
    r.valid = 1;
    rec[t.first + k] = r;
    seg_base[t.first + k] = (unsigned long long)t.seg_base[k];
  }
  if (k == 0 && t.last) seg_base[t.first + t.n] = (unsigned long long)t.seg_base[t.n];
}

__global__ void __launch_bounds__(64) ent_encode_kernel(const EntModel m, const uint8_t* __restrict__ sym,
                                                        const EntRec* __restrict__ rec,
                                                        const unsigned long long* __restrict__ seg_base, int n_streams,
                                                        uint32_t L, uint8_t* __restrict__ slots,
                                                        uint32_t* __restrict__ seg_len) {
  __shared__ uint32_t s_cum[257];
  for (int k = threadIdx.x; k <= m.nsym; k += 64) s_cum[k] = m.cum[k];
  __syncthreads();
  const unsigned long long T = seg_base[n_streams];
  const unsigned long long g = (unsigned long long)blockIdx.x * 64 + threadIdx.x;
  if (g >= T) return;
  const int i = ent_find(seg_base, n_streams, g);
  const unsigned long long j = g - seg_base[i];
  const long long left = rec[i].count - (long long)(j * L);
  const uint32_t cnt = left < (long long)L ? (uint32_t)left : L;
  const uint8_t* src = sym + rec[i].in_off + (long long)(j * L);
  uint32_t* out = reinterpret_cast<uint32_t*>(slots + (size_t)g * ent_stride(L));

  const uint32_t nsym = (uint32_t)m.nsym, total = m.cum[m.nsym];
  const int shift = m.shift;
  unsigned long long low = 0, range = 1ull << 32;
  int cache = -1;
  uint32_t pending = 0, nout = 0, acc = 0;
  bool bad = false;

  auto put = [&](uint32_t b) {
    acc |= (b & 0xFFu) << (8 * (nout & 3));
    ++nout;
    if ((nout & 3) == 0) {
      out[(nout >> 2) - 1] = acc;
      acc = 0;
    }
  };
  auto emit_top = [&]() {
    if (low < 0xFF000000ull || low >= (1ull << 32)) {
      const uint32_t carry = low >= (1ull << 32) ? 1u : 0u;
      if (cache >= 0) put((uint32_t)cache + carry);
      for (; pending; --pending) put(0xFFu + carry);
      cache = (int)((low >> 24) & 0xFF);
    } else {
      ++pending;
    }
    low = (low << 8) & 0xFFFFFFFFull;
  };
  auto step = [&](uint32_t s) {
    if (s >= nsym) {
      bad = true;
      return;
    }
    const uint32_t start = s_cum[s], next = s_cum[s + 1];
    unsigned long long r;
    if (shift >= 0) r = range >> shift;
    else if (range >> 32) r = range / total;
    else r = (uint32_t)range / total;
    const unsigned long long sr = (unsigned long long)start * r;
    low += sr;
    range = next == total ? range - sr : (unsigned long long)(next - start) * r;
    while (range < (1ull << 24)) {
      range <<= 8;
      emit_top();
    }
  };

  uint32_t k = 0;
  for (; k < cnt && ((uintptr_t)(src + k) & 15) != 0; ++k) step(src[k]);
  for (; k + 16 <= cnt; k += 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + k);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t x = w[q];
#pragma unroll 1
      for (int b = 0; b < 4; ++b) {
        step(x & 0xFFu);
        x >>= 8;
      }
    }
  }
  for (; k < cnt; ++k) step(src[k]);

  // the minimal flush (range_coder.cpp EncCore::finish)
  int nb = 0;
  unsigned long long v = low;
  for (; nb <= 4; ++nb) {
    if (nb == 4) {
      v = low;
    } else {
      const unsigned long long unit = 1ull << (32 - 8 * nb);
      v = (low + unit - 1) & ~(unit - 1);
    }
    if (v < low + range) break;
  }
  low = v;
  for (int q = 0; q < nb; ++q) emit_top();
  if (nb > 0) {
    if (cache >= 0) put((uint32_t)cache);
    for (; pending; --pending) put(0xFFu);
  } else if (cache >= 0) {
    const uint32_t carry = v >= (1ull << 32) ? 1u : 0u;
    put((uint32_t)cache + carry);
    for (; pending; --pending) put(0xFFu + carry);
  }
  if (nout & 3) out[nout >> 2] = acc;  // the slot is a multiple of 4 bytes
  seg_len[g] = bad ? kEntBad : nout;
}

// Workgroup i: exclusive scan of stream i's segment lengths; its container size.
__global__ void __launch_bounds__(256) ent_seg_scan_kernel(const EntRec* __restrict__ rec,
                                                           const unsigned long long* __restrict__ seg_base,
                                                           const uint32_t* __restrict__ seg_len,
                                                           unsigned long long* __restrict__ seg_off,
                                                           unsigned long long* __restrict__ sizes) {
  __shared__ unsigned long long s[256];
  __shared__ int s_bad;
  const int i = blockIdx.x, t = threadIdx.x;
  const unsigned long long b = seg_base[i], S = seg_base[i + 1] - b;
  if (t == 0) s_bad = 0;
  __syncthreads();
  unsigned long long carry = 0;
  bool bad = false;
  for (unsigned long long j0 = 0; j0 < S; j0 += 256) {
    const unsigned long long j = j0 + t;
    uint32_t len = j < S ? seg_len[b + j] : 0;
    if (len == kEntBad) {
      bad = true;
      len = 0;
    }
    const unsigned long long inc = ent_block_scan(len, s);
    if (j < S) seg_off[b + j] = carry + inc - len;
    carry += s[255];
    __syncthreads();
  }
  if (bad) s_bad = 1;  // every writer stores the same value
  __syncthreads();
  if (t == 0) sizes[i] = s_bad ? ~0ull : 20ull + 2ull * S + carry;
}

// One workgroup: out[i] = sum of in[k], k < i (UINT64_MAX counts as 0); out has n + 1 entries.
__global__ void __launch_bounds__(256) ent_stream_scan_kernel(const unsigned long long* __restrict__ in, int n,
                                                              unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s[256];
  const int t = threadIdx.x;
  unsigned long long carry = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + t;
    unsigned long long v = i < n ? in[i] : 0;
    if (v == ~0ull) v = 0;
    const unsigned long long inc = ent_block_scan(v, s);
    if (i < n) out[i] = carry + inc - v;
    carry += s[255];
    __syncthreads();
  }
  if (t == 0) out[n] = carry;
}

// Workgroup g: segment g's payload, its length and (first segment) the header to their places.
__global__ void __launch_bounds__(256) ent_gather_kernel(const EntRec* __restrict__ rec,
                                                         const unsigned long long* __restrict__ seg_base,
                                                         int n_streams, uint32_t L, const uint8_t* __restrict__ slots,
                                                         const uint32_t* __restrict__ seg_len,
                                                         const unsigned long long* __restrict__ seg_off,
                                                         const unsigned long long* __restrict__ sizes,
                                                         const unsigned long long* __restrict__ out_off,
                                                         uint8_t* __restrict__ out) {
  const unsigned long long g = blockIdx.x;
  const int i = ent_find(seg_base, n_streams, g);
  if (sizes[i] == ~0ull) return;
  const unsigned long long j = g - seg_base[i], S = seg_base[i + 1] - seg_base[i];
  uint8_t* base = out + out_off[i];
  const int t = threadIdx.x;
  const uint32_t len = seg_len[g];
  if (j == 0 && t < 20) {
    const unsigned long long n = (unsigned long long)rec[i].count;
    uint32_t b;
    if (t < 4) b = (0x53434954u >> (8 * t)) & 0xFFu;  // "TICS"
    else if (t < 8) b = t == 4 ? 1u : 0u;
    else if (t < 12) b = (L >> (8 * (t - 8))) & 0xFFu;
    else b = (uint32_t)(n >> (8 * (t - 12))) & 0xFFu;
    base[t] = (uint8_t)b;
  }
  if (t < 2) base[20 + 2 * j + t] = (uint8_t)(len >> (8 * t));
  const uint8_t* src = slots + (size_t)g * ent_stride(L);
  uint8_t* dst = base + 20 + 2 * S + seg_off[g];
  for (uint32_t k = t; k < len; k += 256) dst[k] = src[k];
}

// Lane k: the header of container first + k against the caller's count and size.
__global__ void __launch_bounds__(64) ent_dec_header_kernel(const EntChunk t, const uint8_t* __restrict__ blob,
                                                            EntRec* __restrict__ rec,
                                                            unsigned long long* __restrict__ seg_cnt) {
  const int k = threadIdx.x;
  if (k >= t.n) return;
  EntRec r;
  r.in_off = t.in_off[k];
  r.in_size = t.in_size[k];
  r.count = t.count[k];
  r.out_off = t.out_off[k];
  r.L = 0;
  r.valid = 0;
  unsigned long long S = 0;
  if (r.in_size >= 20) {
    const uint8_t* p = blob + r.in_off;
    uint32_t L = 0;
    unsigned long long n = 0;
    for (int b = 0; b < 4; ++b) L |= (uint32_t)p[8 + b] << (8 * b);
    for (int b = 0; b < 8; ++b) n |= (unsigned long long)p[12 + b] << (8 * b);
    bool ok = p[0] == 'T' && p[1] == 'I' && p[2] == 'C' && p[3] == 'S' && p[4] == 1 && !p[5] && !p[6] && !p[7];
    ok = ok && L >= 4 && L <= kEntMaxL && (L & 3) == 0 && n == (unsigned long long)r.count;
    if (ok) {
      S = (n + L - 1) / L;
      if (S > (unsigned long long)(r.in_size - 20) / 2) ok = false;
    }
    if (ok) {
      r.L = L;
      r.valid = 1;
    } else {
      S = 0;
    }
  }
  rec[t.first + k] = r;
  seg_cnt[t.first + k] = S;
}

// Workgroup i: the offsets of container i's payloads from its u16 lengths; a container that
// cannot be decoded (header, or its segments do not fit the scratch) becomes zeros.
__global__ void __launch_bounds__(256) ent_dec_scan_kernel(const uint8_t* __restrict__ blob, EntRec* __restrict__ rec,
                                                           const unsigned long long* __restrict__ seg_base,
                                                           unsigned long long cap,
                                                           unsigned long long* __restrict__ seg_off,
                                                           uint8_t* __restrict__ d_sym) {
  __shared__ unsigned long long s[256];
  const int i = blockIdx.x, t = threadIdx.x;
  const EntRec r = rec[i];
  const unsigned long long b = seg_base[i], S = seg_base[i + 1] - b;
  if (!r.valid || b + S > cap) {
    uint8_t* dst = d_sym + r.out_off;
    for (long long k = t; k < r.count; k += 256) dst[k] = 0;
    if (t == 0) rec[i].valid = 0;
    return;
  }
  const uint8_t* lens = blob + r.in_off + 20;
  unsigned long long carry = 20ull + 2ull * S;
  for (unsigned long long j0 = 0; j0 < S; j0 += 256) {
    const unsigned long long j = j0 + t;
    const uint32_t len = j < S ? (uint32_t)lens[2 * j] | (uint32_t)lens[2 * j + 1] << 8 : 0;
    const unsigned long long inc = ent_block_scan(len, s);
    if (j < S) seg_off[b + j] = carry + inc - len;
    carry += s[255];
    __syncthreads();
  }
}

// One segment per lane, grid-stride.  Dynamic LDS: the cumulative table, then (lut != 0) the
// value -> symbol bytes.
__global__ void __launch_bounds__(64) ent_decode_kernel(const EntModel m, int lut, const uint8_t* __restrict__ blob,
                                                        const EntRec* __restrict__ rec,
                                                        const unsigned long long* __restrict__ seg_base, int n_streams,
                                                        const unsigned long long* __restrict__ seg_off,
                                                        uint8_t* __restrict__ d_sym) {
  extern __shared__ uint32_t s_dyn[];
  uint32_t* s_cum = s_dyn;
  uint8_t* s_lut = reinterpret_cast<uint8_t*>(s_dyn + 260);
  const unsigned long long T = seg_base[n_streams];
  if ((unsigned long long)blockIdx.x * 64 >= T) return;
  const int nsym = m.nsym;
  const uint32_t total = m.cum[nsym];
  for (int k = threadIdx.x; k <= nsym; k += 64) s_cum[k] = m.cum[k];
  __syncthreads();
  auto search = [&](uint32_t val) {  // last s with cum[s] <= val
    int lo = 0, hi = nsym - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_cum[mid] <= val) lo = mid;
      else hi = mid - 1;
    }
    return (uint32_t)lo;
  };
  if (lut) {
    for (uint32_t v = threadIdx.x; v < total; v += 64) s_lut[v] = (uint8_t)search(v);
    __syncthreads();
  }
  const int shift = m.shift;

  for (unsigned long long g = (unsigned long long)blockIdx.x * 64 + threadIdx.x; g < T;
       g += (unsigned long long)gridDim.x * 64) {
    const int i = ent_find(seg_base, n_streams, g);
    const EntRec r = rec[i];
    if (!r.valid) continue;
    const unsigned long long j = g - seg_base[i];
    const long long left = r.count - (long long)(j * r.L);
    const uint32_t cnt = left < (long long)r.L ? (uint32_t)left : r.L;
    const uint8_t* cont = blob + r.in_off;
    const uint32_t len = (uint32_t)cont[20 + 2 * j] | (uint32_t)cont[20 + 2 * j + 1] << 8;
    // the segment's extent, clamped to the container
    const unsigned long long size = (unsigned long long)r.in_size;
    unsigned long long pos = seg_off[g];
    if (pos > size) pos = size;
    unsigned long long end = pos + len;
    if (end > size) end = size;
    uint8_t* dst = d_sym + r.out_off + (long long)(j * r.L);

    auto get = [&]() -> uint32_t { return pos < end ? (uint32_t)cont[pos++] : 0u; };
    uint32_t code = 0;
    for (int q = 0; q < 4; ++q) code = (code << 8) | get();
    unsigned long long range = 1ull << 32;
    auto dec = [&]() -> uint32_t {
      unsigned long long rr;
      if (shift >= 0) rr = range >> shift;
      else if (range >> 32) rr = range / total;
      else rr = (uint32_t)range / total;
      uint32_t val = (rr >> 32) ? 0u : code / (uint32_t)rr;
      if (val >= total) val = total - 1;
      const uint32_t s = lut ? (uint32_t)s_lut[val] : search(val);
      const uint32_t start = s_cum[s], next = s_cum[s + 1];
      const unsigned long long sr = (unsigned long long)start * rr;
      code -= (uint32_t)sr;
      range = next == total ? range - sr : (unsigned long long)(next - start) * rr;
      while (range < (1ull << 24)) {
        range <<= 8;
        code = (code << 8) | get();
      }
      return s;
    };

    uint32_t k = 0;
    for (; k < cnt && ((uintptr_t)(dst + k) & 3) != 0; ++k) dst[k] = (uint8_t)dec();
    for (; k + 4 <= cnt; k += 4) {
      uint32_t w = 0;
#pragma unroll 1
      for (int b = 0; b < 4; ++b) w |= dec() << (8 * b);
      *reinterpret_cast<uint32_t*>(dst + k) = w;
    }
    for (; k < cnt; ++k) dst[k] = (uint8_t)dec();
  }
}

}  // namespace tic

namespace {

struct EntState {
  tic::EntModel m;
};
std::mutex g_ent_mu;
std::map<tic_handle*, EntState> g_ent;

// Bytes in front of the per-segment arrays: seg_base[n + 1], a second u64[n + 1] (container
// offsets / segment counts), the records.
size_t ent_fixed(int n) {
  const size_t b = 2 * ((size_t)n + 1) * 8 + (size_t)n * sizeof(tic::EntRec);
  return (b + 15) & ~(size_t)15;
}
bool ent_L_ok(uint32_t L) { return L >= 4 && L <= tic::kEntMaxL && L % 4 == 0; }

// Segments of the list at segment length L, or -1 for a bad count / more than 2^31 - 1.
long long ent_segments(const int64_t* counts, int n, uint32_t L, const char** why) {
  long long T = 0;
  for (int i = 0; i < n; ++i) {
    if (counts[i] <= 0) {
      *why = "every stream needs at least one symbol";
      return -1;
    }
    if (counts[i] > (1ll << 40)) {
      *why = "a stream of more than 2^40 symbols";
      return -1;
    }
    T += (counts[i] + L - 1) / L;
    if (T > INT_MAX) {
      *why = "more than 2^31 - 1 segments";
      return -1;
    }
  }
  return T;
}
size_t ent_scratch(int n, long long T, uint32_t L) {
  const size_t per = (((size_t)T * 12 + 15) & ~(size_t)15);  // seg_off u64, seg_len u32
  return ent_fixed(n) + per + (size_t)T * tic::ent_stride(L);
}

struct EntScratch {
  unsigned long long *seg_base, *aux, *seg_off;
  tic::EntRec* rec;
  uint32_t* seg_len;
  uint8_t* slots;
};
EntScratch ent_carve(void* d_scratch, int n, long long T) {
  EntScratch s;
  uint8_t* p = static_cast<uint8_t*>(d_scratch);
  s.seg_base = reinterpret_cast<unsigned long long*>(p);
  s.aux = s.seg_base + n + 1;
  s.rec = reinterpret_cast<tic::EntRec*>(s.aux + n + 1);
  p += ent_fixed(n);
  s.seg_off = reinterpret_cast<unsigned long long*>(p);
  s.seg_len = reinterpret_cast<uint32_t*>(s.seg_off + T);
  s.slots = p + (((size_t)T * 12 + 15) & ~(size_t)15);
  return s;
}

int ent_model(tic_handle* h, tic::EntModel* m) {
  std::lock_guard<std::mutex> lk(g_ent_mu);
  auto it = g_ent.find(h);
  if (it == g_ent.end()) return fail(TIC_EINVAL, "no entropy table set on this handle (tic_entropy_set_table)");
  *m = it->second.m;
  return TIC_OK;
}

}  // namespace

extern "C" {

void tic_destroy_runtime_(tic_handle* h);

void tic_destroy(tic_handle* h) {
  {
    std::lock_guard<std::mutex> lk(g_ent_mu);
    g_ent.erase(h);
  }
  tic_destroy_runtime_(h);
}

int tic_entropy_set_table(tic_handle* h, const int64_t* cum, size_t ncum) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  // the host coder's own table check: one symbol through tic_rcseg_encode
  const uint8_t zero = 0;
  uint8_t out[32];
  size_t w = 0;
  const int rc = tic_rcseg_encode(&zero, 1, 4, cum, ncum, out, sizeof(out), &w);
  if (rc) return fail(rc, "%s", tic_rc_last_error());
  EntState st;
  memset(&st, 0, sizeof(st));
  st.m.nsym = (int)ncum - 1;
  for (size_t i = 0; i < ncum; ++i) st.m.cum[i] = (uint32_t)cum[i];
  const uint32_t total = st.m.cum[ncum - 1];
  st.m.shift = -1;
  if ((total & (total - 1)) == 0)
    for (int s = 0; s <= 24; ++s)
      if ((1u << s) == total) st.m.shift = s;
  std::lock_guard<std::mutex> lk(g_ent_mu);
  g_ent[h] = st;
  return TIC_OK;
}

int tic_entropy_scratch_bytes(const int64_t* counts, int n_streams, uint32_t L, size_t* bytes) {
  if (!bytes) return fail(TIC_EINVAL, "null bytes");
  *bytes = 0;
  if (n_streams < 0) return fail(TIC_EINVAL, "n_streams %d is negative", n_streams);
  if (n_streams > 0 && !counts) return fail(TIC_EINVAL, "null per-stream array");
  if (!ent_L_ok(L)) return fail(TIC_EINVAL, "segment length %u must be a multiple of 4 in [4, 16384]", L);
  const char* why = "";
  const long long T = ent_segments(counts, n_streams, L, &why);
  if (T < 0) return fail(TIC_EINVAL, "%s", why);
  *bytes = ent_scratch(n_streams, T, L);
  return TIC_OK;
}

int tic_entropy_encode_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets, const int64_t* counts,
                              int n_streams, uint32_t L, void* d_scratch, size_t scratch_bytes, uint8_t* d_out,
                              size_t out_cap, uint64_t* d_sizes) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (n_streams < 0) return fail(TIC_EINVAL, "n_streams %d is negative", n_streams);
  if (n_streams == 0) return TIC_OK;
  if (!d_sym || !d_scratch || !d_out || !d_sizes) return fail(TIC_EINVAL, "null device pointer");
  if (!sym_offsets || !counts) return fail(TIC_EINVAL, "null per-stream array");
  if (!ent_L_ok(L)) return fail(TIC_EINVAL, "segment length %u must be a multiple of 4 in [4, 16384]", L);
  const char* why = "";
  const long long T = ent_segments(counts, n_streams, L, &why);
  if (T < 0) return fail(TIC_EINVAL, "%s", why);
  size_t bound = 0;
  for (int i = 0; i < n_streams; ++i) {
    if (sym_offsets[i] < 0) return fail(TIC_EINVAL, "stream %d: negative offset %lld", i, (long long)sym_offsets[i]);
    const size_t S = ((size_t)counts[i] + L - 1) / L;
    bound += 20 + 2 * S + 3 * (size_t)counts[i] + 4 * S;
  }
  tic::EntModel m;
  int rc = ent_model(h, &m);
  if (rc) return rc;
  if (((uintptr_t)d_scratch & 15) != 0 || ((uintptr_t)d_sizes & 7) != 0)
    return fail(TIC_EINVAL, "d_scratch must be 16-byte and d_sizes 8-byte aligned");
  const size_t need = ent_scratch(n_streams, T, L);
  if (scratch_bytes < need)
    return fail(TIC_EINVAL, "scratch of %zu bytes is too small (tic_entropy_scratch_bytes: %zu)", scratch_bytes, need);
  if (out_cap < bound)
    return fail(TIC_EINVAL, "out_cap %zu is below the sum of tic_rcseg_bound (%zu)", out_cap, bound);

  HIP_TRY(hipSetDevice(h->device));
  const EntScratch s = ent_carve(d_scratch, n_streams, T);
  long long segs = 0;
  for (int f = 0; f < n_streams; f += tic::kEntStreams) {
    tic::EntChunk t;
    memset(&t, 0, sizeof(t));
    t.n = std::min(tic::kEntStreams, n_streams - f);
    t.first = f;
    t.last = f + t.n == n_streams;
    for (int k = 0; k < t.n; ++k) {
      t.in_off[k] = sym_offsets[f + k];
      t.count[k] = counts[f + k];
      t.seg_base[k] = segs;
      segs += (counts[f + k] + L - 1) / L;
    }
    t.seg_base[t.n] = segs;
    touch(h);
    hipLaunchKernelGGL(tic::ent_put_kernel, dim3(1), dim3(64), 0, h->stream, t, L, s.rec, s.seg_base);
    if ((rc = check_launch())) return rc;
  }
  const unsigned wgs = (unsigned)((T + 63) / 64);
  hipLaunchKernelGGL(tic::ent_encode_kernel, dim3(wgs), dim3(64), 0, h->stream, m, d_sym, (const tic::EntRec*)s.rec,
                     (const unsigned long long*)s.seg_base, n_streams, L, s.slots, s.seg_len);
  if ((rc = check_launch())) return rc;
  unsigned long long* sizes = reinterpret_cast<unsigned long long*>(d_sizes);
  hipLaunchKernelGGL(tic::ent_seg_scan_kernel, dim3((unsigned)n_streams), dim3(256), 0, h->stream,
                     (const tic::EntRec*)s.rec, (const unsigned long long*)s.seg_base, (const uint32_t*)s.seg_len,
                     s.seg_off, sizes);
  if ((rc = check_launch())) return rc;
  hipLaunchKernelGGL(tic::ent_stream_scan_kernel, dim3(1), dim3(256), 0, h->stream, (const unsigned long long*)sizes,
                     n_streams, s.aux);
  if ((rc = check_launch())) return rc;
  hipLaunchKernelGGL(tic::ent_gather_kernel, dim3((unsigned)T), dim3(256), 0, h->stream, (const tic::EntRec*)s.rec,
                     (const unsigned long long*)s.seg_base, n_streams, L, (const uint8_t*)s.slots,
                     (const uint32_t*)s.seg_len, (const unsigned long long*)s.seg_off,
                     (const unsigned long long*)sizes, (const unsigned long long*)s.aux, d_out);
  return check_launch();
}

int tic_entropy_decode_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                              const int64_t* blob_sizes, const int64_t* counts, int n_streams, uint8_t* d_sym,
                              const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (n_streams < 0) return fail(TIC_EINVAL, "n_streams %d is negative", n_streams);
  if (n_streams == 0) return TIC_OK;
  if (!d_blob || !d_scratch || !d_sym) return fail(TIC_EINVAL, "null device pointer");
  if (!blob_offsets || !blob_sizes || !counts || !sym_offsets) return fail(TIC_EINVAL, "null per-stream array");
  const char* why = "";
  const long long Tmin = ent_segments(counts, n_streams, tic::kEntMaxL, &why);
  if (Tmin < 0) return fail(TIC_EINVAL, "%s", why);
  for (int i = 0; i < n_streams; ++i)
    if (blob_offsets[i] < 0 || blob_sizes[i] < 0 || sym_offsets[i] < 0)
      return fail(TIC_EINVAL, "stream %d: negative offset or size", i);
  tic::EntModel m;
  int rc = ent_model(h, &m);
  if (rc) return rc;
  if (((uintptr_t)d_scratch & 15) != 0) return fail(TIC_EINVAL, "d_scratch must be 16-byte aligned");
  const size_t fixed = ent_fixed(n_streams);
  if (scratch_bytes < fixed + (size_t)Tmin * 8)
    return fail(TIC_EINVAL, "scratch of %zu bytes is too small (tic_entropy_scratch_bytes)", scratch_bytes);
  // segments the scratch has room for: the containers' own L decides how many there are
  const unsigned long long cap = std::min<unsigned long long>((scratch_bytes - fixed) / 8, INT_MAX);

  const uint32_t total = m.cum[m.nsym];
  const int lut = total <= tic::kEntLutMax;
  const size_t lds = 260 * sizeof(uint32_t) + (lut ? ((size_t)total + 3) / 4 * 4 : 0);
  HIP_TRY(hipSetDevice(h->device));
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(tic::ent_decode_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const EntScratch s = ent_carve(d_scratch, n_streams, 0);
  for (int f = 0; f < n_streams; f += tic::kEntStreams) {
    tic::EntChunk t;
    memset(&t, 0, sizeof(t));
    t.n = std::min(tic::kEntStreams, n_streams - f);
    t.first = f;
    for (int k = 0; k < t.n; ++k) {
      t.in_off[k] = blob_offsets[f + k];
      t.in_size[k] = blob_sizes[f + k];
      t.count[k] = counts[f + k];
      t.out_off[k] = sym_offsets[f + k];
    }
    touch(h);
    hipLaunchKernelGGL(tic::ent_dec_header_kernel, dim3(1), dim3(64), 0, h->stream, t, d_blob, s.rec, s.aux);
    if ((rc = check_launch())) return rc;
  }
  hipLaunchKernelGGL(tic::ent_stream_scan_kernel, dim3(1), dim3(256), 0, h->stream, (const unsigned long long*)s.aux,
                     n_streams, s.seg_base);
  if ((rc = check_launch())) return rc;
  hipLaunchKernelGGL(tic::ent_dec_scan_kernel, dim3((unsigned)n_streams), dim3(256), 0, h->stream, d_blob, s.rec,
                     (const unsigned long long*)s.seg_base, cap, s.seg_off, d_sym);
  if ((rc = check_launch())) return rc;
  const unsigned wgs = (unsigned)std::min<unsigned long long>((cap + 63) / 64, 1u << 16);
  hipLaunchKernelGGL(tic::ent_decode_kernel, dim3(wgs), dim3(64), lds, h->stream, m, lut, d_blob,
                     (const tic::EntRec*)s.rec, (const unsigned long long*)s.seg_base, n_streams,
                     (const unsigned long long*)s.seg_off, d_sym);
  return check_launch();
}

}  // extern "C"
